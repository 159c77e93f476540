"""Multi-session streaming CLI: many file-driven sessions converted concurrently, chunk by chunk, through one
MultiStreamConverter (module/multistream.py) -- one batched device step per tick for all of them.

The sessions file is a JSON list; each entry:
  {"input": "a.wav",                      the session's input
   "target": "spk.wav" and / or "lib": "voice_library.pt",   its voice (as -t / -lib of realtime_inference.py)
   "pitch": 0, "f0_rate": 1, "alpha": 0, "gain": 0, "input_gain": 0,     optional, realtime_inference.py's meanings
   "world_pitch": false,                  optional, a JSON bool: realtime_inference.py's -wpe (WORLD's f0 of the ring; its
                                          f0_rate is then not applied, as there)
   "k": 4,                                optional, an integer in 1..8: the session's own k (default: -k)
   "auto_pitch": false,                   optional, a JSON bool (default: --auto-pitch): the pitch shift follows the target
                                          voice's register (module/multistream.py "Auto pitch"); "pitch" is then an offset on top
   "register_hz": 180,                    optional: declares the register (mean f0 in Hz) of a voice given by "lib" alone, which
                                          has no audio to measure it on; a "target" wav's register is measured at enrolment
   "intonation": 1.0,                     optional, a number >= 0 (default: -int): the session's pitch excursions around its running
                                          mean pitch are scaled by it (module/multistream.py "Pitch range")
   "auto_range": false,                   optional, a JSON bool (default: --auto-range): the excursions are also scaled so that the
                                          source's running standard deviation meets the target voice's
   "range_st": 2.5,                       optional, beside "register_hz": declares the pitch range (standard deviation in semitones)
                                          of a voice given by "lib" alone; a "target" wav's range is measured at enrolment
   "pitch_track": true,                   optional, a JSON bool (default: -pt): the session's f0 is the Viterbi path over the f0
                                          estimator's class scores of its ring instead of their per-frame argmax
                                          (module/multistream.py "Pitch tracking"); not with "world_pitch"
   "match_path": true, "path_weight": 1,  optional, a JSON bool (default: -mp) and a number >= 0 (default: --path-weight): each frame's
                                          matched feature is ONE of its k nearest rows, chosen by a Viterbi path over the ring
                                          (MultiStreamConverter.open(match_path=, path_weight=))
   "track_weight": 1, "track_jump": 12,   optional, numbers >= 0 (defaults: --track-weight / --track-jump): the tracker's cost per
                                          semitone moved inside the band and its flat cost of any other move
   "voicing": true,                       optional, a JSON bool (default: -vd): the session's f0 is 0 on the frames of its ring that are
                                          not periodic (module/multistream.py "Voicing"); not with "world_pitch"
   "voicing_on": 0.6, "voicing_off": 0.45, "voicing_floor_db": -60,      optional (defaults: --voicing-on / --voicing-off /
                                          --voicing-floor): the session's two thresholds on the normalised correlation and its silence floor
   "gate_db": -40, "gate_hold": 0.2,      optional: the session's input gate (module/multistream.py "Input gate"): a threshold in
                                          dBFS on its 16 kHz ring after the input gain (null: no gate; default -thr) and the
                                          seconds it stays open after the last loud tick (default --gate-hold)
   "crossfade_ms": 10,                    optional, a number of milliseconds > 0 or null (default: --crossfade): the head of every
                                          chunk of the session is faded in from the previous tick's continuation over that long
                                          (module/multistream.py "Seam crossfade"; at most the session's chunk; needs -isr == -osr)
   "limit_db": -1, "limit_lookahead_ms": 5, "limit_hold_ms": 20,     optional: the session's output limiter (module/multistream.py
                                          "Limiter"): a ceiling in dBFS <= 0 that no emitted sample exceeds (null: no limiter;
                                          default -lim), the milliseconds over which the gain falls ahead of a peak (at most the
                                          session's chunk; default --limit-lookahead) and those it stays down after one (default
                                          --limit-hold)
   "lufs": -23,                           optional, a number of LUFS in (-70, 0] or null (default: -lufs): what the session emits is
                                          brought to this loudness by a running ITU-R BS.1770 measurement and a slewed gain, ahead of
                                          the limiter (module/multistream.py "Loudness"); null: the session's level is left alone
   "envelope": 0.7,                       optional, a number in [0, 1] or null (default: -env): how far the session's converted voice
                                          follows the loudness contour of its input (module/multistream.py "Envelope follow"); 0 or
                                          null: the decoder's own level
   "post_filter": 0.8,                    optional, a number in [0, 0.85] or null (default: -pf): the alpha of the session's adaptive
                                          formant post filter, right after the decoder and ahead of "envelope" (module/multistream.py
                                          "Post filter"); 0 or null: no filter
   "codebook": 4096,                      optional, an integer >= 1 or null (default: --codebook): the session's voice is condensed to
                                          that many centroid rows by k-means when it is packed or enrolled (module/codebook.py); a
                                          voice of that many rows or fewer stays as it is.  A codebook's rows are means: use k 1 or 2
   "blend": [{"target": "a.wav", "weight": 2}, {"lib": "b.pt", "weight": 1}],   instead of "target" / "lib": a weighted mix
                                          of 1 to 4 voices, each component a voice source as above (multistream.blend_spec)
   "start": 0,                            optional: the tick at which the session joins
   "stall": [12, 13, 40],                 optional, a list of distinct integers >= 0: ticks, counted from tick 0 of the run, at which
                                          the session supplies nothing (a late client; module/multistream.py "Sparse ticks").  Its
                                          remaining input moves later by one tick per stall, and its slot closes after its last chunk
   "lose": [20, 21],                      optional, a list of distinct integers >= 0: ticks, counted from tick 0 of the run, at which
                                          the session's next input chunk is consumed and DROPPED: it never arrives, but the session's
                                          clock goes on (module/multistream.py "Lost chunks"), so the output keeps its length -- this is
                                          not a stall.  A tick named in both "lose" and "stall" is an error
   "conceal": true,                       optional, a JSON bool (default: on in a concealing converter): whether the session's lost
                                          chunks are concealed by waveform substitution; false: they are chunks of zeros
   "sr": 48000,                           optional: the session's sample rate (default -isr / -osr)
   "output": "a_out.wav"}                 optional: default <outdir>/<index>_<input name>.wav
A session's slot opens at its start tick, gets one chunk per tick while its input lasts and closes after its last chunk.
A session with "sr" has its input resampled to sr on load, is driven at sr in chunks of chunk * sr / isr samples (a whole number,
with the converter's 16 kHz geometry: module/multistream.py session_geometry), and its output wav is written at sr.  "sr" needs
-isr == -osr.
The converter carries the WORLD branch only if some session asks for "world_pitch": a sessions file without it runs as before.
It is built with blend = the most components of any session's "blend" (1 without one: a file without blends runs as before);
sessions and blend components naming the same voice sources share one voice of the pool.
It is built with k_max = the largest "k" only if some session's "k" differs from -k (converter_k_max): a file without "k" runs as
before.  Sessions on one voice at different k take one pass over that voice per k.
The converter carries the auto-pitch kernel, and the voices are given registers (measured with the f0 estimator on the target wavs),
only if some session is on auto pitch: a file without "auto_pitch", run without --auto-pitch, runs as before.
The converter is built with pitch_range=True, and the voices are given registers and ranges, only if some session ends up at an
"intonation" other than 1 or on "auto_range" (or under -int / --auto-range): a file without the keys, run without the flags, runs as
before.
The converter carries the voicing kernels only if some session ends up deciding ("voicing", or -vd): a file without the key, run
without the flag, runs as before.  --voicing-lo / --voicing-hi hold for the whole converter.
The converter stores the class scores and carries the tracker kernel only if some session ends up tracking ("pitch_track", or -pt): a
file without the key, run without the flag, runs as before.  --track-lo / --track-hi / --track-band hold for the whole converter.
The converter carries the two gate kernels only if some session ends up gated ("gate_db", or -thr): a file without the keys, run
without -thr, runs as before.
The converter carries the seam kernel only if some session ends up with a crossfade ("crossfade_ms", or --crossfade): a file without
the key, run without the flag, runs as before.
The converter carries the limiter kernel only if some session ends up limited ("limit_db", or -lim): a file without the key, run
without the flag, runs as before.
The converter carries the loudness kernel only if some session ends up normalised ("lufs", or -lufs): a file without the key, run
without the flag, runs as before.  --loudness-half-life / --loudness-prior / --loudness-gate / --loudness-max-db / --loudness-slew hold
for the whole converter.
The converter carries the envelope kernel only if some session ends up following ("envelope" above 0, or -env): a file without the
key, run without the flag, runs as before.  Likewise the post filter kernel ("post_filter" above 0, or -pf; --post-filter-ratio /
--post-filter-tilt hold for the whole converter).
The voices are condensed only for sessions with a "codebook" (or under --codebook): a file without the key, run without the flag, runs
as before.  The size is part of the voice's pool name: sessions on the same sources at different sizes get different voices; a blend's
components are each condensed to the session's size.
WORLD needs rings of about 230 ms or more (-c 960 -b 8 is 480 ms): a shorter ring comes out unvoiced.
Flags shared with realtime_inference.py keep its spelling: -c, -b, -k, -isr, -osr, --no-graph.

The converter is built sparse (rings on the device, sessions may sit ticks out) only under --sparse or if some session has a
"stall": a file without the key, run without the flag, runs as before.  A stalled session's output is byte for byte what it is
without the stalls, and --sparse alone writes byte for byte what a run without it writes.

The converter conceals lost chunks (and is then sparse) only under --conceal or if some session has a "lose" or a true "conceal": a
file without the keys, run without the flag, runs as before; "lose": [] and --conceal alone write byte for byte what a run without
them writes.  --conceal-hold / --conceal-fade / --conceal-recover set the three durations for all sessions.

--pool-rows N: a RESERVED pool of N rows (module/multistream.py VoicePool(capacity=N)) instead of one packed before tick 0: each
voice is enrolled from its sources at the first tick some session needs it (multistream.enrol_voice, while the other sessions
run) and removed after the last session on it closes, so N need only cover the voices alive at one time (enrol_plan lists the
enrolments, the removals and the peak).  The pool is compacted when a voice fits its free rows but none of its holes; a voice
that does not fit ends the run with the pool's `add` error before any audio is written.  The outputs are byte for byte those
without the flag.

--pool-dtype fp16: the pool stores its rows in half precision (VoicePool(dtype=torch.float16); 1536 bytes per row instead of 3072),
with or without --pool-rows; the sessions file is the same.  Every voice's tokens are rounded to fp16 as they are enrolled, and the
run writes byte for byte what an fp32 pool of the rounded tokens writes.  Default fp32: the pool and the run are what they were.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from module import audio_io, common                             # noqa: E402
from module.content_encoder import ContentEncoder                # noqa: E402
from module.decoder import Decoder                               # noqa: E402
from module.f0_estimator import F0Estimator                      # noqa: E402
from module.multistream import (MultiStreamConverter, POOL_DTYPES, VoicePool, blend_sources, check_k, enrol_voice,   # noqa: E402
                                check_conceal_ms, check_crossfade_ms, check_envelope, check_intonation, check_limit, check_post_filter,
                                check_loudness, check_loudness_stream,
                                gate_hold_ticks, gate_thr_ms, measure_register)
from module.spectrogram import spectrogram                       # noqa: E402
from module.voice_library import VoiceLibrary                    # noqa: E402

SESSION_KEYS = ("input", "target", "lib", "pitch", "f0_rate", "alpha", "gain", "input_gain", "world_pitch", "start", "sr", "output",
                "blend", "k", "auto_pitch", "register_hz")
GATE_KEYS = ("gate_db", "gate_hold")     # taken per session too; a loaded session carries them only when it is gated
SEAM_KEYS = ("crossfade_ms",)            # taken per session too; a loaded session carries it only when it crossfades
LIMIT_KEYS = ("limit_db", "limit_lookahead_ms", "limit_hold_ms")      # likewise; a loaded session carries them only when it limits
POSTFILTER_KEYS = ("post_filter",)       # likewise; a loaded session carries it only when it is filtered (an alpha above 0)
ENVELOPE_KEYS = ("envelope",)            # likewise; a loaded session carries it only when it follows (an amount above 0)
LOUDNESS_KEYS = ("lufs",)                # likewise; a loaded session carries it only when it is normalised
CODEBOOK_KEYS = ("codebook",)            # taken per session too; a loaded session carries it only when its voice is condensed
STALL_KEYS = ("stall",)                  # a loaded session carries it only when its entry has the key (the converter is then sparse)
LOSE_KEYS = ("lose",)                    # likewise (the converter is then sparse and conceals)
CONCEAL_KEYS = ("conceal",)              # likewise: the session's own switch
RANGE_KEYS = ("intonation", "auto_range")    # a loaded session carries "intonation" only when it is not 1, "auto_range" only when on
TRACK_KEYS = ("pitch_track", "track_weight", "track_jump")      # a loaded session carries them only when it tracks
PATH_KEYS = ("match_path", "path_weight")                       # a loaded session carries them only when its match takes the path
VOICING_KEYS = ("voicing", "voicing_on", "voicing_off", "voicing_floor_db")      # likewise: only when it decides
RANGE_ST_KEYS = ("range_st",)            # a loaded session carries it only when its entry has the key


def build_parser():
    parser = argparse.ArgumentParser(description="Convert many voices concurrently")
    parser.add_argument('sessions', help="JSON list of sessions (see the module docstring)")
    parser.add_argument('-o', '--output-dir', default="outputs")
    parser.add_argument('-d', '--device', default='cuda', choices=['cpu', 'cuda', 'mps'])
    parser.add_argument('-dep', '--decoder-path', default="decoder.pt")
    parser.add_argument('-cep', '--content-encoder-path', default="content_encoder.pt")
    parser.add_argument('-f0ep', '--f0-estimator-path', default="f0_estimator.pt")
    parser.add_argument('-b', '--buffersize', default=8, type=int)
    parser.add_argument('-c', '--chunk', default=960, type=int)
    parser.add_argument('-k', default=4, type=int)
    parser.add_argument('-isr', '--input-sr', default=16000, type=int)
    parser.add_argument('-osr', '--output-sr', default=16000, type=int)
    parser.add_argument('--slots', default=0, type=int, help="session slots of the converter (default: one per session)")
    parser.add_argument('--pool-rows', default=None, type=int,
                        help="a reserved voice pool of this many rows: voices are enrolled at the first tick that needs them and "
                             "removed after their last session (default: every voice is packed before tick 0)")
    parser.add_argument('--pool-dtype', default="fp32", choices=sorted(POOL_DTYPES),
                        help="the element type of the pool's row table: fp16 halves its bytes, the tokens are rounded as they are "
                             "enrolled (default fp32)")
    parser.add_argument('--auto-pitch', action='store_true',
                        help="sessions follow their target voice's register unless their \"auto_pitch\" says otherwise")
    parser.add_argument('-int', '--intonation', default=1.0, type=float,
                        help="sessions scale their pitch excursions around their running mean pitch by this factor unless their "
                             "\"intonation\" says otherwise (default 1: off)")
    parser.add_argument('--auto-range', action='store_true',
                        help="sessions match their target voice's pitch range unless their \"auto_range\" says otherwise")
    parser.add_argument('-thr', '--gate-db', default=None, type=float,
                        help="input gate: sessions mute (and skip their search) below this level in dBFS unless their \"gate_db\" "
                             "says otherwise (default: no gate)")
    parser.add_argument('--gate-hold', default=0.2, type=float,
                        help="seconds a gate stays open after the last loud tick (default 0.2; a session's \"gate_hold\" overrides)")
    parser.add_argument('--crossfade', default=None, type=float, metavar="MS",
                        help="seam crossfade: sessions fade the head of every chunk in from the previous tick's continuation over "
                             "MS milliseconds unless their \"crossfade_ms\" says otherwise (default: hard cuts)")
    parser.add_argument('-lim', '--limit', default=None, type=float, metavar="DB",
                        help="output limiter: no emitted sample exceeds this ceiling in dBFS (<= 0), so the 16-bit edge never wraps; the "
                             "gain starts to fall --limit-lookahead before a peak unless a session's \"limit_db\" says otherwise (default: no limiter)")
    parser.add_argument('--limit-lookahead', default=5.0, type=float, metavar="MS",
                        help="milliseconds over which the limiter's gain falls ahead of a peak and recovers after the hold (default 5; a session's \"limit_lookahead_ms\" overrides)")
    parser.add_argument('--limit-hold', default=20.0, type=float, metavar="MS",
                        help="milliseconds the limiter's gain stays down after a peak (default 20; a session's \"limit_hold_ms\" overrides)")
    parser.add_argument('-lufs', '--lufs', default=None, type=float, metavar="L",
                        help="loudness normalisation: what every session emits is brought to this loudness in LUFS (ITU-R BS.1770, -70 < L "
                             "<= 0) by a running measurement and a slewed gain, ahead of the limiter, unless its \"lufs\" says otherwise "
                             "(module/multistream.py \"Loudness\"; default: the level is left alone)")
    parser.add_argument('--loudness-half-life', default=3.0, type=float, metavar="S",
                        help="seconds after which a 400-ms block counts half in a session's running loudness (default 3)")
    parser.add_argument('--loudness-prior', default=1.0, type=float, metavar="S",
                        help="seconds of counted blocks until a session's running loudness is trusted in full (default 1)")
    parser.add_argument('--loudness-gate', default=-70.0, type=float, metavar="LUFS",
                        help="the absolute gate under which a block is not counted (default -70)")
    parser.add_argument('--loudness-max-db', default=12.0, type=float, metavar="DB",
                        help="the most the loudness gain turns a session up or down (default 12)")
    parser.add_argument('--loudness-slew', default=6.0, type=float, metavar="DB",
                        help="the most the loudness gain moves per second, in dB (default 6)")
    parser.add_argument('-pf', '--post-filter-alpha', default=0.0, type=float, metavar="A",
                        help="adaptive formant post filter on the sessions' converted waves, ahead of -env: the alpha of the denominator, 0 "
                             "(off, the default) to 0.85, unless their \"post_filter\" says otherwise (module/multistream.py \"Post filter\")")
    parser.add_argument('--post-filter-ratio', default=0.625, type=float, metavar="R",
                        help="the post filter's numerator alpha as a share of the denominator's, 0 to 1 (default 0.625)")
    parser.add_argument('--post-filter-tilt', default=0.5, type=float, metavar="T",
                        help="the share of the post filter's spectral tilt that is taken out again, 0 to 1 (default 0.5)")
    parser.add_argument('-env', '--envelope', default=0.0, type=float, metavar="A",
                        help="envelope follow: the sessions' converted voices take on their inputs' loudness contours by this amount, 0 (off, the "
                             "default) to 1, unless their \"envelope\" says otherwise (module/multistream.py \"Envelope follow\").  It can "
                             "lift samples above full scale: use -lim beside it")
    parser.add_argument('--envelope-floor', default=-60.0, type=float, metavar="DB",
                        help="the level under which the envelope follow stops telling the two signals apart (default -60)")
    parser.add_argument('--envelope-range', default=12.0, type=float, metavar="DB",
                        help="the most the envelope follow turns a frame up or down (default 12)")
    parser.add_argument('--envelope-radius', default=1, type=int, metavar="FRAMES",
                        help="20 ms frames on each side over which the envelope follow smooths both levels, 0 to 4 (default 1: 60 ms)")
    parser.add_argument('--codebook', default=None, type=int, metavar="SIZE",
                        help="condense every session's voice to SIZE centroid rows by k-means unless its \"codebook\" says otherwise "
                             "(default: the voices as they are)")
    parser.add_argument('--sparse', action='store_true',
                        help="build the converter sparse: the rings live on the device and a session may sit ticks out (implied by a "
                             "session's \"stall\")")
    parser.add_argument('--conceal', action='store_true',
                        help="build the converter sparse and concealing: a session's lost chunks (\"lose\") are filled by waveform "
                             "substitution unless its \"conceal\" says otherwise (implied by a session's \"lose\")")
    parser.add_argument('--conceal-hold', default=10.0, type=float, metavar="MS",
                        help="milliseconds a concealed loss repeats the last pitch period at full level (default 10)")
    parser.add_argument('--conceal-fade', default=50.0, type=float, metavar="MS",
                        help="milliseconds over which a longer loss then fades to silence (default 50)")
    parser.add_argument('--conceal-recover', default=5.0, type=float, metavar="MS",
                        help="milliseconds over which the first chunk after a loss is faded in from the concealment (default 5)")
    parser.add_argument('--no-graph', action='store_true',
                        help="launch the per-tick device pipeline kernel by kernel instead of replaying one captured hipGraph")
    common.add_track_arguments(parser)      # (-pt: sessions track unless their "pitch_track" says otherwise)
    common.add_path_arguments(parser)       # (-mp: sessions take the match path unless their "match_path" says otherwise)
    common.add_voicing_arguments(parser)    # (-vd: sessions decide unless their "voicing" says otherwise)
    return parser


def register_hz_of(entry, where):
    """an entry's "register_hz" (None without one): a number > 0, for a voice given by "lib" alone"""
    hz = entry.get("register_hz")
    if hz is None:
        return None
    if isinstance(hz, bool) or not isinstance(hz, (int, float)) or not 0 < hz < float("inf"):
        raise ValueError(f"{where}: \"register_hz\" must be a number > 0, got {hz!r}")
    if "blend" in entry or entry.get("target") is not None or entry.get("lib") is None:
        raise ValueError(f"{where}: \"register_hz\" declares the register of a voice given by \"lib\" alone (a \"target\" wav's is "
                         "measured; a blend's comes from its voices)")
    return float(hz)


def range_st_of(entry, where):
    """an entry's "range_st" (None without one): a number of semitones > 0, for a voice given by "lib" alone"""
    st = entry.get("range_st")
    if st is None:
        return None
    if isinstance(st, bool) or not isinstance(st, (int, float)) or not 0 < st < float("inf"):
        raise ValueError(f"{where}: \"range_st\" must be a number of semitones > 0, got {st!r}")
    if "blend" in entry or entry.get("target") is not None or entry.get("lib") is None:
        raise ValueError(f"{where}: \"range_st\" declares the pitch range of a voice given by \"lib\" alone (a \"target\" wav's is "
                         "measured; a blend's comes from its voices)")
    if entry.get("register_hz") is None:
        raise ValueError(f"{where}: \"range_st\" goes beside \"register_hz\": a range is declared around a declared register")
    return float(st)


def declared_ranges(entries, name_of):
    """{voice name: semitones} of the entries' "range_st"; ValueError if two entries declare different ones for one voice"""
    out = {}
    for i, e in enumerate(entries):
        if e.get("range_st") is not None:
            name = name_of(e)
            if out.setdefault(name, e["range_st"]) != e["range_st"]:
                raise ValueError(f"entry {i}: \"range_st\" {e['range_st']} but an earlier entry gave this voice {out[name]}")
    return out


def session_range(s, where, intonation=1.0, auto_range=False):
    """an entry's pitch range settings -> (intonation, auto_range): "intonation" (default `intonation`) a finite number >= 0,
    "auto_range" (default `auto_range`) a JSON bool; ValueError otherwise"""
    it, on = s.get("intonation", intonation), s.get("auto_range", bool(auto_range))
    if not isinstance(on, bool):
        raise ValueError(f"{where}: \"auto_range\" must be true or false, got {on!r}")
    try:
        return check_intonation(it, "\"intonation\""), on
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None


def session_path(s, where, match_path=False, weight=common.PATH_WEIGHT):
    """an entry's match path settings -> the weight as a float, or None for a session whose match takes no path: "match_path" (default
    `match_path`) a JSON bool, "path_weight" (default `weight`) a number >= 0; ValueError otherwise"""
    on = s.get("match_path", bool(match_path))
    if not isinstance(on, bool):
        raise ValueError(f"{where}: \"match_path\" must be true or false, got {on!r}")
    try:
        w = common.path_param(s.get("path_weight", weight), "\"path_weight\"")
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return w if on else None


def session_track(s, where, pitch_track=False, weight=common.TRACK_WEIGHT, jump=common.TRACK_JUMP):
    """an entry's tracker settings -> (weight, jump) as floats, or None for a session that does not track: "pitch_track" (default
    `pitch_track`) a JSON bool, "track_weight" / "track_jump" (defaults `weight`, `jump`) numbers >= 0; ValueError otherwise, and
    together with "world_pitch" """
    on = s.get("pitch_track", bool(pitch_track))
    if not isinstance(on, bool):
        raise ValueError(f"{where}: \"pitch_track\" must be true or false, got {on!r}")
    try:
        w, j = (common.track_param("\"track_weight\"", s.get("track_weight", weight)),
                common.track_param("\"track_jump\"", s.get("track_jump", jump)))
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    if not on:
        return None
    if s.get("world_pitch", False):
        raise ValueError(f"{where}: \"pitch_track\" cannot be combined with \"world_pitch\"")
    return w, j


def session_voicing(s, where, voicing=False, on=common.VOICING_ON, off=common.VOICING_OFF, floor_db=common.VOICING_FLOOR_DB):
    """an entry's voicing settings -> (on, off, floor_db) as floats, or None for a session that does not decide: "voicing" (default
    `voicing`) a JSON bool, "voicing_on" / "voicing_off" / "voicing_floor_db" (defaults `on`, `off`, `floor_db`) numbers with
    0 < off <= on <= 1; ValueError otherwise, and together with "world_pitch" """
    v = s.get("voicing", bool(voicing))
    if not isinstance(v, bool):
        raise ValueError(f"{where}: \"voicing\" must be true or false, got {v!r}")
    o = common.voicing_options(dict(on=s.get("voicing_on", on), off=s.get("voicing_off", off),
                                    floor_db=s.get("voicing_floor_db", floor_db)), where)
    if not v:
        return None
    if s.get("world_pitch", False):
        raise ValueError(f"{where}: \"voicing\" cannot be combined with \"world_pitch\"")
    return o["on"], o["off"], o["floor_db"]


def declared_registers(entries, name_of):
    """{voice name: Hz} of the entries' "register_hz"; ValueError if two entries declare different ones for one voice"""
    out = {}
    for i, e in enumerate(entries):
        if e.get("register_hz") is not None:
            name = name_of(e)
            if out.setdefault(name, e["register_hz"]) != e["register_hz"]:
                raise ValueError(f"entry {i}: \"register_hz\" {e['register_hz']} but an earlier entry gave this voice {out[name]}")
    return out


def session_gate(s, where, gate_db=None, gate_hold=0.2):
    """an entry's gate -> (gate_db, gate_hold), or None for a session without a gate: "gate_db" (default `gate_db`; a JSON null
    switches the gate off) a finite number, "gate_hold" (default `gate_hold`) a finite number >= 0; ValueError otherwise"""
    db, hold = s.get("gate_db", gate_db), s.get("gate_hold", gate_hold)
    try:
        gate_hold_ticks(hold, 1.0)
        if db is not None:
            gate_thr_ms(db)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return None if db is None else (float(db), float(hold))


def session_crossfade(s, where, crossfade_ms=None):
    """an entry's "crossfade_ms" (default `crossfade_ms`) -> a float > 0, or None for a session with hard cuts (a JSON null switches
    the default off); ValueError otherwise"""
    try:
        return check_crossfade_ms(s.get("crossfade_ms", crossfade_ms))
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None


def session_limit(s, where, limit_db=None, lookahead_ms=5.0, hold_ms=20.0):
    """an entry's limiter -> (limit_db, limit_lookahead_ms, limit_hold_ms) as floats, or None for a session without one: "limit_db"
    (default `limit_db`; a JSON null switches the limiter off) a finite number <= 0, "limit_lookahead_ms" (default `lookahead_ms`) a
    finite number > 0, "limit_hold_ms" (default `hold_ms`) a finite number >= 0; ValueError otherwise"""
    db, look, hold = s.get("limit_db", limit_db), s.get("limit_lookahead_ms", lookahead_ms), s.get("limit_hold_ms", hold_ms)
    try:
        checked = check_limit(db, look, hold)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return None if checked is None else (float(db), checked[1], checked[2])


def session_loudness(s, where, lufs=None):
    """an entry's "lufs" (default `lufs`; a JSON null switches the default off) -> a float in (-70, 0], or None for a session whose
    level is left alone; ValueError otherwise"""
    target = s.get("lufs", lufs)
    try:
        check_loudness(target)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return None if target is None else float(target)


def session_envelope(s, where, envelope=0.0, floor_db=-60.0, range_db=12.0, radius=1):
    """an entry's "envelope" (default `envelope`; a JSON null or 0 switches the default off) -> the amount as a float in (0, 1], or
    None for a session that does not follow; ValueError otherwise (the three tuning values are those of the flags, checked with it)"""
    a = s.get("envelope", envelope)
    try:
        a = check_envelope(0.0 if a is None else a, floor_db, range_db, radius)[0]
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return a if a > 0 else None


def session_post_filter(s, where, alpha=0.0, ratio=0.625, tilt=0.5):
    """an entry's "post_filter" (default `alpha`; a JSON null or 0 switches the default off) -> the alpha as a float in (0, 0.85], or
    None for a session that is not filtered; ValueError otherwise (ratio and tilt are those of the flags, checked with it)"""
    a = s.get("post_filter", alpha)
    try:
        a = check_post_filter(0.0 if a is None else a, ratio, tilt)[0]
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return a if a > 0 else None


def session_codebook(s, where, codebook=None):
    """an entry's "codebook" (default `codebook`) -> an integer >= 1, or None for a voice that stays as it is (a JSON null switches
    the default off); ValueError otherwise"""
    size = s.get("codebook", codebook)
    if size is None:
        return None
    if isinstance(size, bool) or not isinstance(size, int) or size < 1:
        raise ValueError(f"{where}: \"codebook\" must be an integer >= 1 or null, got {size!r}")
    return size


def session_stall(s, where):
    """an entry's "stall" -> the sorted tuple of its ticks, or None for a session without the key (a JSON null counts as none): a list
    of distinct integers >= 0 (no bools, no floats); ValueError otherwise.  Host only"""
    stall = s.get("stall")
    if stall is None:
        return None
    if not isinstance(stall, list) or any(isinstance(t, bool) or not isinstance(t, int) or t < 0 for t in stall):
        raise ValueError(f"{where}: \"stall\" must be a list of distinct integers >= 0 (ticks of the run), got {stall!r}")
    if len(set(stall)) != len(stall):
        raise ValueError(f"{where}: \"stall\" names a tick twice: {stall!r}")
    return tuple(sorted(stall))


def session_lose(s, where):
    """an entry's "lose" -> the sorted tuple of its ticks, or None for a session without the key (a JSON null counts as none): a list
    of distinct integers >= 0 (no bools, no floats), none of them one of its "stall" ticks; ValueError otherwise.  Host only"""
    lose = s.get("lose")
    if lose is None:
        return None
    if not isinstance(lose, list) or any(isinstance(t, bool) or not isinstance(t, int) or t < 0 for t in lose):
        raise ValueError(f"{where}: \"lose\" must be a list of distinct integers >= 0 (ticks of the run), got {lose!r}")
    if len(set(lose)) != len(lose):
        raise ValueError(f"{where}: \"lose\" names a tick twice: {lose!r}")
    both = sorted(set(lose) & set(session_stall(s, where) or ()))
    if both:
        raise ValueError(f"{where}: ticks {both} are named in both \"lose\" and \"stall\": a tick's chunk is late or it is lost")
    return tuple(sorted(lose))


def session_conceal(s, where):
    """an entry's "conceal" -> a bool, or None for a session without the key (a JSON null counts as none); ValueError otherwise"""
    v = s.get("conceal")
    if v is not None and not isinstance(v, bool):
        raise ValueError(f"{where}: \"conceal\" must be true or false, got {v!r}")
    return v


def supply_ticks(start, n_chunks, stall=None):
    """the ticks at which a session that joins at tick `start` supplies its n_chunks chunks, in order: every tick from `start` on
    that is not one of its `stall` ticks (without stalls: start .. start + n_chunks - 1).  Host only"""
    stall, out, tick = set(stall or ()), [], int(start)
    while len(out) < n_chunks:
        if tick not in stall:
            out.append(tick)
        tick += 1
    return out


def load_sessions(path, k=4, auto_pitch=False, gate_db=None, gate_hold=0.2, codebook=None, crossfade_ms=None, limit_db=None,
                  limit_lookahead_ms=5.0, limit_hold_ms=20.0, envelope=0.0, envelope_floor_db=-60.0, envelope_range_db=12.0,
                  envelope_radius=1, conceal_hold_ms=10.0, conceal_fade_ms=50.0, conceal_recover_ms=5.0, intonation=1.0,
                  auto_range=False, pitch_track=False, track_weight=common.TRACK_WEIGHT, track_jump=common.TRACK_JUMP, lufs=None,
                  voicing=False, voicing_on=common.VOICING_ON, voicing_off=common.VOICING_OFF, voicing_floor_db=common.VOICING_FLOOR_DB,
                  match_path=False, path_weight=common.PATH_WEIGHT, post_filter=0.0, post_filter_ratio=0.625, post_filter_tilt=0.5):
    """the sessions file -> list of dicts with every key filled in ("k": the session's own, default `k`; "auto_pitch": default
    `auto_pitch`); a gated session ("gate_db", default `gate_db`) also carries "gate_db" and "gate_hold", a session without a gate
    neither, so a file without the keys loads to what it did; likewise "codebook" (default `codebook`) only on a session whose voice is
    condensed, "crossfade_ms" (default `crossfade_ms`) only on a session that crossfades, and "limit_db" / "limit_lookahead_ms" /
    "limit_hold_ms" (defaults `limit_db`, `limit_lookahead_ms`, `limit_hold_ms`) only on a session that limits, "envelope" (default
    `envelope`) only on a session that follows at an amount above 0, and "stall" (a sorted
    tuple of ticks) only on a session whose entry has the key, as "lose" (a sorted tuple of ticks) and "conceal" (a bool); "intonation"
    (default `intonation`) only on a session whose factor is not 1, "auto_range" (default `auto_range`) only on one that is on, and
    "range_st" only where the entry has it; "pitch_track" (true), "track_weight" and "track_jump" (defaults `pitch_track`,
    `track_weight`, `track_jump`) only on a session that tracks; "lufs" (default `lufs`) only on a session that is normalised;
    "voicing" (true), "voicing_on", "voicing_off" and "voicing_floor_db" (defaults `voicing`, `voicing_on`, `voicing_off`,
    `voicing_floor_db`) only on a session that decides; "match_path" (true) and "path_weight" (defaults `match_path`, `path_weight`)
    only on a session whose match takes the path; "post_filter" (default `post_filter`) only on a session that is filtered at an
    alpha above 0; ValueError on a malformed entry"""
    session_path({}, "-mp / --path-weight", match_path, path_weight)
    session_voicing({}, "-vd / --voicing-on / --voicing-off / --voicing-floor", voicing, voicing_on, voicing_off, voicing_floor_db)
    session_track({}, "-pt / --track-weight / --track-jump", pitch_track, track_weight, track_jump)
    try:
        check_conceal_ms(conceal_hold_ms, conceal_fade_ms, conceal_recover_ms)
    except ValueError as e:
        raise ValueError(f"--conceal-hold / --conceal-fade / --conceal-recover: {e}") from None
    k = check_k(k, "-k")
    session_codebook({}, "--codebook", codebook)
    session_gate({}, "-thr / --gate-hold", gate_db, gate_hold)
    session_crossfade({}, "--crossfade", crossfade_ms)
    session_limit({}, "-lim / --limit-lookahead / --limit-hold", limit_db, limit_lookahead_ms, limit_hold_ms)
    env = (envelope_floor_db, envelope_range_db, envelope_radius)
    session_envelope({}, "-env / --envelope-floor / --envelope-range / --envelope-radius", envelope, *env)
    pf = (post_filter_ratio, post_filter_tilt)
    session_post_filter({}, "-pf / --post-filter-ratio / --post-filter-tilt", post_filter, *pf)
    session_range({}, "-int / --auto-range", intonation, auto_range)
    session_loudness({}, "-lufs", lufs)
    with open(path) as f:
        sessions = json.load(f)
    if not isinstance(sessions, list) or not sessions:
        raise ValueError(f"{path}: expected a non-empty JSON list of sessions")
    base = os.path.dirname(os.path.abspath(path))
    out = []
    for i, s in enumerate(sessions):
        if not isinstance(s, dict) or "input" not in s:
            raise ValueError(f"session {i}: an object with an \"input\" wav is required")
        unknown = (set(s) - set(SESSION_KEYS) - set(GATE_KEYS) - set(SEAM_KEYS) - set(LIMIT_KEYS) - set(ENVELOPE_KEYS) - set(CODEBOOK_KEYS)
                   - set(STALL_KEYS) - set(LOSE_KEYS) - set(CONCEAL_KEYS) - set(RANGE_KEYS) - set(RANGE_ST_KEYS) - set(TRACK_KEYS) - set(VOICING_KEYS)
                   - set(LOUDNESS_KEYS) - set(PATH_KEYS) - set(POSTFILTER_KEYS))
        if unknown:
            raise ValueError(f"session {i}: unknown keys {sorted(unknown)} (known: "
                             f"{SESSION_KEYS + GATE_KEYS + SEAM_KEYS + LIMIT_KEYS + ENVELOPE_KEYS + CODEBOOK_KEYS + STALL_KEYS + LOSE_KEYS + CONCEAL_KEYS + RANGE_KEYS + RANGE_ST_KEYS + TRACK_KEYS + LOUDNESS_KEYS + VOICING_KEYS + PATH_KEYS + POSTFILTER_KEYS})")
        gate = session_gate(s, f"session {i}", gate_db, gate_hold)
        xf = session_crossfade(s, f"session {i}", crossfade_ms)
        size = session_codebook(s, f"session {i}", codebook)
        lim = session_limit(s, f"session {i}", limit_db, limit_lookahead_ms, limit_hold_ms)
        amount = session_envelope(s, f"session {i}", envelope, *env)
        pfa = session_post_filter(s, f"session {i}", post_filter, *pf)
        target = session_loudness(s, f"session {i}", lufs)
        rel = lambda p: None if p is None else (p if os.path.isabs(p) else os.path.join(base, p))      # noqa: E731
        blend = blend_sources(s, f"session {i}", rel) if "blend" in s else None
        if blend is None and s.get("target") is None and s.get("lib") is None:
            raise ValueError(f"session {i}: needs a \"target\" wav or a \"lib\" voice library")
        if not isinstance(s.get("world_pitch", False), bool):
            raise ValueError(f"session {i}: \"world_pitch\" must be true or false, got {s['world_pitch']!r}")
        if not isinstance(s.get("auto_pitch", False), bool):
            raise ValueError(f"session {i}: \"auto_pitch\" must be true or false, got {s['auto_pitch']!r}")
        sess_k = check_k(s["k"], f"session {i}: \"k\"") if "k" in s else k
        stall = session_stall(s, f"session {i}")
        lose, con = session_lose(s, f"session {i}"), session_conceal(s, f"session {i}")
        inton, ranged = session_range(s, f"session {i}", intonation, auto_range)
        range_st = range_st_of(s, f"session {i}")
        track = session_track(s, f"session {i}", pitch_track, track_weight, track_jump)
        decide = session_voicing(s, f"session {i}", voicing, voicing_on, voicing_off, voicing_floor_db)
        path_w = session_path(s, f"session {i}", match_path, path_weight)
        e = dict(input=rel(s["input"]), target=rel(s.get("target")), lib=rel(s.get("lib")), output=rel(s.get("output")),
                 pitch=float(s.get("pitch", 0.0)), f0_rate=float(s.get("f0_rate", 1.0)), alpha=float(s.get("alpha", 0.0)),
                 gain=float(s.get("gain", 0.0)), input_gain=float(s.get("input_gain", 0.0)), start=int(s.get("start", 0)),
                 sr=None if s.get("sr") is None else int(s["sr"]), world_pitch=s.get("world_pitch", False), blend=blend, k=sess_k,
                 auto_pitch=s.get("auto_pitch", bool(auto_pitch)), register_hz=register_hz_of(s, f"session {i}"))
        if e["start"] < 0:
            raise ValueError(f"session {i}: start tick {e['start']} < 0")
        if e["sr"] is not None and e["sr"] <= 0:
            raise ValueError(f"session {i}: sample rate {e['sr']} <= 0")
        if gate is not None:
            e["gate_db"], e["gate_hold"] = gate
        if xf is not None:
            e["crossfade_ms"] = xf
        if lim is not None:
            e["limit_db"], e["limit_lookahead_ms"], e["limit_hold_ms"] = lim
        if amount is not None:
            e["envelope"] = amount
        if pfa is not None:
            e["post_filter"] = pfa
        if target is not None:
            e["lufs"] = target
        if size is not None:
            e["codebook"] = size
        if stall is not None:
            e["stall"] = stall
        if lose is not None:
            e["lose"] = lose
        if con is not None:
            e["conceal"] = con
        if inton != 1.0:
            e["intonation"] = inton
        if ranged:
            e["auto_range"] = True
        if range_st is not None:
            e["range_st"] = range_st
        if track is not None:
            e["pitch_track"], (e["track_weight"], e["track_jump"]) = True, track
        if decide is not None:
            e["voicing"], (e["voicing_on"], e["voicing_off"], e["voicing_floor_db"]) = True, decide
        if path_w is not None:
            e["match_path"], e["path_weight"] = True, path_w
        out.append(e)
    return out


def voice_name(target, lib, codebook=None):
    """the pool name of a voice source: sessions and blend components with the same sources share one voice -- at the same codebook
    size: the size is part of the name (none: the name it always had)"""
    return json.dumps([target, lib] if codebook is None else [target, lib, codebook])


def session_voice(s):
    """the session's voice for MultiStreamConverter.open: a pool name, or (name, weight) pairs for a blend"""
    if s.get("blend"):
        return [(voice_name(t, lb, s.get("codebook")), w) for t, lb, w in s["blend"]]
    return voice_name(s["target"], s["lib"], s.get("codebook"))


def blend_size(sessions):
    """the converter's blend: the most components of any session's blend, 1 for a file without blends"""
    return max([len(s["blend"]) for s in sessions if s.get("blend")] or [1])


def converter_k_max(sessions, k):
    """MultiStreamConverter's k_max: None (the uniform converter, as before) unless some session's k differs from the default
    `k`; then the largest k in use, the default included"""
    ks = [s.get("k", k) for s in sessions]
    return None if all(v == k for v in ks) else max(ks + [k])


def session_sources(s):
    """the (target, lib) voice sources a session uses: its own, or its blend's components"""
    return [(t, lb) for t, lb, _ in s["blend"]] if s.get("blend") else [(s["target"], s["lib"])]


def enrol_plan(sessions):
    """The --pool-rows schedule as pure host logic.  `sessions`: dicts with "start" (its first tick), "ticks" (how many it runs;
    0: it never opens) and "voices" ({pool name: rows}, blend components included).  A voice is enrolled before the first tick
    that some session needs it and removed after the last tick of the last session on it (and enrolled again if a later session
    asks for it after that).  Returns (events, peak): events is the list of (tick, "enrol" | "remove", name) in the order in which
    they happen -- a tick's enrolments come before its step, its removals after it -- and peak the most rows alive at one time."""
    first, last = {}, {}
    live = [s for s in sessions if s["ticks"] > 0]
    ticks = sorted({s["start"] for s in live} | {s["start"] + s["ticks"] - 1 for s in live})
    events, rows, users, alive, peak = [], {}, {}, 0, 0
    for tick in ticks:
        for s in live:
            if s["start"] == tick:
                for name, m in s["voices"].items():
                    if rows.setdefault(name, m) != m:
                        raise ValueError(f"voice {name!r} is given {rows[name]} and {m} rows")
                    if users.get(name, 0) == 0:
                        events.append((tick, "enrol", name))
                        alive += m
                    users[name] = users.get(name, 0) + 1
        peak = max(peak, alive)
        for s in live:
            if s["start"] + s["ticks"] - 1 == tick:
                for name, m in s["voices"].items():
                    users[name] -= 1
                    if users[name] == 0:
                        events.append((tick, "remove", name))
                        alive -= m
    return events, peak


def voice_tokens(ce, target, lib, device):
    """a session's library as realtime_inference.py builds it: the target utterance's frames (every 4th) and / or a library file"""
    tgt = torch.zeros(1, 768, 0, device=device)
    if target is not None:
        wf, sr = audio_io.load(target)
        wf = audio_io.resample(wf.to(device), sr, 16000)
        wf = wf / wf.abs().max()
        tgt = ce(spectrogram(wf[:1]))[:, :, ::4]
    if lib is not None:
        VL = VoiceLibrary().to(device)
        VL.load_state_dict(torch.load(lib, map_location=device))
        tgt = torch.cat([tgt, VL.tokens], dim=2)
    return tgt[0].contiguous()


def condensed(tokens, codebook):
    """the voice's tokens [768, M] as they go into the pool: its `codebook`-row codebook (None: as they are)"""
    if codebook is None:
        return tokens
    from module.codebook import build_codebook
    return build_codebook(tokens, codebook)


def voice_tokens_register(ce, pe, target, lib, device):
    """voice_tokens and the voice's register (sum of voiced pitch, voiced frames), measured with the f0 estimator on the same 16 kHz
    audio the content encoder sees (multistream.measure_register); None for a voice without a target wav"""
    register = None
    if target is not None:
        wf, sr = audio_io.load(target)
        wf = audio_io.resample(wf.to(device), sr, 16000)
        wf = wf / wf.abs().max()
        register = measure_register(pe, wf[:1].contiguous())
    return voice_tokens(ce, target, lib, device), register


def input_pcm(path, input_sr, device):
    wf, sr = audio_io.load(path)
    wf = audio_io.resample(wf.mean(dim=0, keepdim=True).to(device), sr, input_sr)[0].cpu()
    return (wf.numpy() * 32767).astype(np.int16)


def run(conv, pcms, starts, chunk, params, before=None, after=None, stalls=None, loses=None):
    """drive `conv` tick by tick: session i occupies slot i (opened with params[i]) from tick starts[i] for len(pcms[i]) // chunk
    ticks; `chunk` is one length for every session or a list of per-session lengths (sessions at their own rates).
    before(tick) runs ahead of the tick's opens and after(tick) behind its closes (--pool-rows: enrolments and removals).
    stalls (a sparse converter): per session the ticks at which it supplies nothing, or None; it then supplies its chunks at
    supply_ticks(start, chunks, stall) and its slot closes after the last of them.
    loses (a concealing converter): per session the ticks at which the chunk it would supply is consumed and dropped (step's lost=),
    or None; a tick at which the session supplies nothing anyway counts for nothing.
    Returns the emitted int16 chunks of every session, concatenated."""
    chunks = list(chunk) if isinstance(chunk, (list, tuple)) else [chunk] * len(pcms)
    n_chunks = [len(p) // c for p, c in zip(pcms, chunks)]
    outs = [[] for _ in pcms]
    supply = [{t: j for j, t in enumerate(supply_ticks(s, n, st))}
              for s, n, st in zip(starts, n_chunks, stalls or [None] * len(pcms))]
    # a session's last tick; one without a single chunk never opens and counts as before: up to its start, "closed" the tick before
    ends = [max(sup) if sup else s - 1 for sup, s in zip(supply, starts)]
    last = max(e + 1 for e in ends)
    for tick in range(last):
        if before is not None:
            before(tick)
        feed, lost = {}, []
        for i, (s, n) in enumerate(zip(starts, n_chunks)):
            if tick == s and n > 0:
                conv.open(i, **params[i])
            if tick in supply[i]:
                j, c = supply[i][tick], chunks[i]
                if loses is not None and loses[i] is not None and tick in loses[i]:
                    lost.append(i)
                else:
                    feed[i] = pcms[i][j * c:(j + 1) * c]
        res = conv.step(feed, lost) if lost else conv.step(feed)
        for i, o in res.items():
            if o is not None:
                outs[i].append(o)
        for i, e in enumerate(ends):
            if tick == e:
                conv.close(i)
        if after is not None:
            after(tick)
    return [np.concatenate(o) if o else np.zeros(0, np.int16) for o in outs]


def make_pool(args, device):
    """the run's (still empty) voice pool: reserved under --pool-rows, of --pool-dtype"""
    return VoicePool(device=device, capacity=args.pool_rows, dtype=POOL_DTYPES[args.pool_dtype])


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        tw, tj, lo, hi, band = common.track_arguments(args)             # (before anything is loaded)
        voicing_opts = common.voicing_options(dict(lo=args.voicing_lo, hi=args.voicing_hi), "--voicing-lo / --voicing-hi")
        common.path_arguments(args)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    sessions = load_sessions(args.sessions, args.k, args.auto_pitch, args.gate_db, args.gate_hold, args.codebook,
                             args.crossfade, args.limit, args.limit_lookahead, args.limit_hold, args.envelope, args.envelope_floor,
                             args.envelope_range, args.envelope_radius, args.conceal_hold, args.conceal_fade, args.conceal_recover,
                             args.intonation, args.auto_range, args.pitch_track, tw, tj, args.lufs, args.voicing, args.voicing_on,
                             args.voicing_off, args.voicing_floor, args.match_path, args.path_weight, args.post_filter_alpha,
                             args.post_filter_ratio, args.post_filter_tilt)
    loud = dict(loudness_half_life=args.loudness_half_life, loudness_prior=args.loudness_prior, loudness_gate_lufs=args.loudness_gate,
                loudness_max_db=args.loudness_max_db, loudness_slew_db=args.loudness_slew)
    try:
        check_loudness_stream(*loud.values())                           # (before anything is loaded)
    except ValueError as e:
        raise SystemExit(f"Error: {e}") from None
    if any(s["sr"] is not None for s in sessions) and args.input_sr != args.output_sr:
        raise SystemExit(f"Error: sessions with their own \"sr\" need -isr == -osr (got {args.input_sr} and {args.output_sr})")
    if args.device != 'cuda' or not torch.cuda.is_available():
        raise SystemExit("Error: this build needs a ROCm device: pass -d cuda on an MI355X host.")
    device = torch.device('cuda')
    PE, CE, Dec = F0Estimator().to(device), ContentEncoder().to(device), Decoder().to(device)
    PE.load_state_dict(torch.load(args.f0_estimator_path, map_location=device))
    CE.load_state_dict(torch.load(args.content_encoder_path, map_location=device))
    Dec.load_state_dict(torch.load(args.decoder_path, map_location=device))

    # auto pitch: only then are the voices' registers measured (with the f0 estimator) or declared ("register_hz")
    # pitch range: likewise the converter is built with pitch_range=True, and the voices measured, only if some session needs it
    wants_range = any("intonation" in s or "auto_range" in s for s in sessions)
    ranged = any("auto_range" in s for s in sessions)
    on_auto = any(s["auto_pitch"] for s in sessions)
    auto = on_auto or ranged                            # (the voices' registers, and with them their ranges, are measured)
    name_of = lambda s: voice_name(s["target"], s["lib"], s.get("codebook"))      # noqa: E731
    declared = declared_registers(sessions, name_of) if auto else {}
    declared_st = declared_ranges(sessions, name_of) if ranged else {}
    pool, names = make_pool(args, device), []
    for s in sessions:
        for target, lib in session_sources(s):
            name = voice_name(target, lib, s.get("codebook"))
            if args.pool_rows is None and name not in pool.segments:
                if auto:
                    tokens, register = voice_tokens_register(CE, PE, target, lib, device)
                    pool.add(name, condensed(tokens, s.get("codebook")), register)
                    if name in declared:
                        pool.set_register(name, hz=declared[name], range_st=declared_st.get(name))
                else:
                    pool.add(name, condensed(voice_tokens(CE, target, lib, device), s.get("codebook")))
        names.append(session_voice(s))
    slots = max(args.slots, len(sessions))
    in_sr = [s["sr"] or args.input_sr for s in sessions]
    out_sr = [s["sr"] or args.output_sr for s in sessions]
    conceal = args.conceal or any("lose" in s or s.get("conceal") for s in sessions)      # (a concealing converter is sparse)
    conv = MultiStreamConverter(CE, PE, Dec, pool, slots, chunk=args.chunk, buffersize=args.buffersize, input_sr=args.input_sr,
                                output_sr=args.output_sr, k=args.k, device=device, rates=sorted(set(in_sr)),
                                world_pitch=any(s["world_pitch"] for s in sessions), blend=blend_size(sessions),
                                k_max=converter_k_max(sessions, args.k), auto_pitch=on_auto,
                                **(dict(pitch_range=True) if wants_range else {}),
                                **(dict(pitch_track=True, track_lo=lo, track_hi=hi, track_band=band)
                                   if any("pitch_track" in s for s in sessions) else {}),
                                **(dict(voicing=True, voicing_lo=voicing_opts["lo"], voicing_hi=voicing_opts["hi"])
                                   if any("voicing" in s for s in sessions) else {}),
                                **(dict(match_path=True) if any("match_path" in s for s in sessions) else {}),
                                **(dict(gate=True) if any("gate_db" in s for s in sessions) else {}),
                                **(dict(crossfade=True) if any("crossfade_ms" in s for s in sessions) else {}),
                                **(dict(limiter=True) if any("limit_db" in s for s in sessions) else {}),
                                **(dict(loudness=True, **loud) if any("lufs" in s for s in sessions) else {}),
                                **(dict(envelope=True, envelope_floor_db=args.envelope_floor, envelope_range_db=args.envelope_range,
                                        envelope_radius=args.envelope_radius) if any("envelope" in s for s in sessions) else {}),
                                **(dict(post_filter=True, post_filter_ratio=args.post_filter_ratio, post_filter_tilt=args.post_filter_tilt)
                                   if any("post_filter" in s for s in sessions) else {}),
                                **(dict(sparse=True) if args.sparse or conceal or any("stall" in s for s in sessions) else {}),
                                **(dict(conceal=True, conceal_hold_ms=args.conceal_hold, conceal_fade_ms=args.conceal_fade,
                                        conceal_recover_ms=args.conceal_recover) if conceal else {}))
    params = [dict(voice=n, pitch=s["pitch"], f0_rate=s["f0_rate"], alpha=s["alpha"], gain=s["gain"],
                   input_gain=s["input_gain"], rate=r, world_pitch=s["world_pitch"], k=s["k"], auto_pitch=s["auto_pitch"],
                   **{g: s[g] for g in GATE_KEYS + SEAM_KEYS + LIMIT_KEYS + ENVELOPE_KEYS + CONCEAL_KEYS + RANGE_KEYS + TRACK_KEYS
                      + LOUDNESS_KEYS + VOICING_KEYS + PATH_KEYS + POSTFILTER_KEYS if g in s})
              for n, s, r in zip(names, sessions, in_sr)]
    if not args.no_graph:
        conv.enable_graph()
    pcms = [input_pcm(s["input"], r, device) for s, r in zip(sessions, in_sr)]
    chunks = [args.chunk * r // args.input_sr for r in in_sr]
    before = after = None
    if args.pool_rows is not None:
        # the reserved pool: a tick's first sessions on a voice enrol it ahead of their open, its last one's close removes it
        n_ticks = [len(p) // c for p, c in zip(pcms, chunks)]
        # (a stalled session occupies its slot, and holds its voices, until its last chunk: its stalls lengthen its life)
        n_ticks = [supply_ticks(s["start"], n, s.get("stall"))[-1] - s["start"] + 1 if n else 0 for s, n in zip(sessions, n_ticks)]
        sources = {voice_name(t, lb, s.get("codebook")): (t, lb, s.get("codebook")) for s in sessions for t, lb in session_sources(s)}
        events, _ = enrol_plan([dict(start=s["start"], ticks=n,
                                     voices={voice_name(t, lb, s.get("codebook")): 1 for t, lb in session_sources(s)})
                                for s, n in zip(sessions, n_ticks)])

        def before(tick):
            for name in [n for t, what, n in events if t == tick and what == "enrol"]:
                target, lib, size = sources[name]
                wav, sr = audio_io.load(target) if target is not None else (None, None)
                enrol_voice(pool, name, CE, wav, sr, lib=lib, compact=True, f0_estimator=PE if auto else None, codebook=size)
                if name in declared:
                    pool.set_register(name, hz=declared[name], range_st=declared_st.get(name))

        def after(tick):
            for name in [n for t, what, n in events if t == tick and what == "remove"]:
                pool.remove(name)
    stalls = [s.get("stall") for s in sessions]
    loses = [s.get("lose") for s in sessions]
    outs = run(conv, pcms, [s["start"] for s in sessions], chunks, params, before, after,
               **(dict(stalls=stalls) if any(st is not None for st in stalls) else {}),
               **(dict(loses=loses) if any(ls is not None for ls in loses) else {}))
    os.makedirs(args.output_dir, exist_ok=True)
    for i, (s, o, r) in enumerate(zip(sessions, outs, out_sr)):
        path = s["output"] or os.path.join(args.output_dir, f"{i}_{os.path.splitext(os.path.basename(s['input']))[0]}.wav")
        audio_io.save(path, torch.from_numpy(o.astype(np.float32) / 32768)[None], r, "pcm16")
        print(f"session {i}: {len(o)} samples -> {path}")
    return outs


if __name__ == "__main__":
    main()
