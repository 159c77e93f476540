"""Many-to-many batch conversion CLI: a corpus of files, each converted to a voice of its own, in ONE batched run
(module/pipeline.py: Converter.convert_many -- the windows of every file form one batch, the kNN match is one pool search).

The jobs file is a JSON list; each entry:
  {"input": "a.wav",                                        the file to convert
   "target": "spk.wav" and / or "lib": "voice_library.pt",  its voice (as -t / -lib of inference.py; both: concatenated in
                                                            inference.py's order, the target's frames first)
   "pitch": 0, "intonation": 1, "f0_rate": 1, "alpha": 0,   optional, inference.py's -p / -int / -f0 / -a
   "gain": 1, "normalize": false,                           optional, inference.py's -g / -norm
   "world_pitch": false,                                    optional, a JSON bool: inference.py's -wpe (WORLD's f0 of each
                                                            window; pitch, intonation and f0_rate apply to it)
   "k": 4,                                                  optional, an integer in 1..8: this job's k (default: -k).  Jobs at
                                                            different k still share the one batched run (the pool search groups
                                                            its rows by voice and k); a jobs file without "k" runs as before
   "auto_pitch": false,                                     optional, a JSON bool (default: --auto-pitch): the pitch shift follows
                                                            the target voice's register (convert_many(auto_pitch=)): the voice's
                                                            mean pitch minus this file's, measured on the device; "pitch" is then
                                                            an offset on top.  A jobs file without it runs as before
   "register_hz": 180,                                      optional: declares the register (mean f0 in Hz) of a voice given by
                                                            "lib" alone; a "target" wav's register is measured when it is encoded
   "auto_range": false,                                     optional, a JSON bool (default: --auto-range): the file's pitch
                                                            excursions are scaled around its own mean pitch so that its standard
                                                            deviation meets the target voice's (convert_many(auto_range=)), on top of
                                                            "intonation".  A jobs file without it runs as before
   "range_st": 2.5,                                         optional, beside "register_hz": declares the pitch range (standard
                                                            deviation in semitones) of a voice given by "lib" alone
   "limit_db": -1,                                          optional, a number of dBFS <= 0 or null (default: -lim): the output
                                                            limiter (module/multistream.py limit_waves) on the device after the
                                                            gain, at the file's own rate, before "normalize": no sample exceeds
                                                            the ceiling.  A jobs file without it, run without -lim, runs as before
   "lufs": -23,                                             optional, a number of LUFS in (-70, 0] or null (default: -lufs): the
                                                            file is brought to this integrated loudness (ITU-R BS.1770-4;
                                                            module/multistream.py normalize_loudness) by one gain within
                                                            --loudness-max-db dB, on the device after the gain, at the file's own
                                                            rate, before "limit_db" and "normalize".  A jobs file without it, run
                                                            without -lufs, runs as before
   "envelope": 0.7,                                         optional, a number in [0, 1] or null (default: -env): how far the converted
                                                            voice follows the source's loudness contour (module/multistream.py
                                                            follow_envelope), at 16 kHz before the output resample and the gain; 0 or
                                                            null: the decoder's own level.  A jobs file without it, run without -env,
                                                            runs as before
   "post_filter": 0.8,                                      optional, a number in [0, 0.85] or null (default: -pf): the alpha of the
                                                            adaptive formant post filter (module/multistream.py post_filter) on the
                                                            converted wave at 16 kHz, ahead of "envelope"; 0 or null: no filter.  A
                                                            jobs file without it, run without -pf, runs as before
   "pitch_track": true,                                     optional, a JSON bool or {"weight": 1, "jump": 12} (default: -pt with
                                                            --track-weight / --track-jump): the file's f0 is the Viterbi path over
                                                            the f0 estimator's class scores of each window instead of their argmax
                                                            (convert_many(pitch_track=); inference.py's -pt).  Not with
                                                            "world_pitch".  --track-lo / --track-hi / --track-band hold for the
                                                            whole run.  A jobs file without it, run without -pt, runs as before
   "voicing": true,                                         optional, a JSON bool or {"on": 0.6, "off": 0.45, "floor_db": -60} (default:
                                                            -vd with --voicing-on / --voicing-off / --voicing-floor): the file's f0
                                                            is 0 on the frames whose source is not periodic (convert_many(voicing=);
                                                            inference.py's -vd).  Not with "world_pitch".  --voicing-lo /
                                                            --voicing-hi hold for the whole run.  A jobs file without it, run
                                                            without -vd, runs as before
   "match_path": true,                                      optional, a JSON bool or {"weight": 1} (default: -mp with --path-weight):
                                                            each frame's matched feature is ONE of its k nearest rows, chosen by a
                                                            Viterbi path over each window (convert_many(match_path=); inference.py's
                                                            -mp).  A jobs file without it, run without -mp, runs as before
   "blend": [{"target": "a.wav", "weight": 2},              instead of "target" / "lib": a weighted mix of 1 to 4 voices, each
             {"lib": "b.pt", "weight": 1}],                 component a voice source as above (module/multistream.py blend_spec)
   "output": "a_out.wav"}                                   optional: default <outdir>/<index>_<input name>.wav
Jobs and blend components naming the same voice sources share one voice of the pool.  Every file keeps inference.py's edges:
loaded, resampled to 16 kHz, normalised by its maximum, mono mean; the output resampled back to the file's own rate, gain, optional normalisation.
Each output is bitwise what `inference.py --knn-strict` (with `-wpe True` for a WORLD job) writes for that file, voice and
settings; WORLD and estimator jobs mix freely in one run.
Flags shared with inference.py keep its spelling: -c, -k, -d, -dep, -cep, -f0ep, --window-batch, --pcm16, --no-trim-context.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from module import audio_io, common                             # noqa: E402
from module.multistream import MAX_K, blend_sources, check_k     # noqa: E402

JOB_KEYS = ("input", "target", "lib", "pitch", "intonation", "f0_rate", "alpha", "gain", "normalize", "world_pitch", "output",
            "blend", "k", "auto_pitch", "register_hz")
ENVELOPE_KEYS = ("envelope",)            # likewise; a loaded job carries it only when it follows (an amount above 0)
POSTFILTER_KEYS = ("post_filter",)       # likewise; a loaded job carries it only when it is filtered (an alpha above 0)
LIMIT_KEYS = ("limit_db",)               # taken per job too; a loaded job carries it only when it is limited
LOUDNESS_KEYS = ("lufs",)                # likewise; a loaded job carries it only when it is normalised
TRACK_KEYS = ("pitch_track",)            # a loaded job carries it only when it tracks: {"weight": W, "jump": J}
VOICING_KEYS = ("voicing",)              # a loaded job carries it only when it decides: {"on": R, "off": R, "floor_db": DB}
PATH_KEYS = ("match_path",)              # a loaded job carries it only when its match takes a path: {"weight": W}
RANGE_KEYS = ("auto_range", "range_st")  # a loaded job carries "auto_range" only when it is on, "range_st" only when its entry has it


def build_parser():
    parser = argparse.ArgumentParser(description="Convert many files, each to its own voice, in one batched run")
    parser.add_argument('jobs', help="JSON list of jobs (see the module docstring)")
    parser.add_argument('-o', '--outputs', default="./outputs/")
    parser.add_argument('-d', '--device', default='cuda')
    parser.add_argument('-dep', '--decoder-path', default="decoder.pt")
    parser.add_argument('-cep', '--content-encoder-path', default="content_encoder.pt")
    parser.add_argument('-f0ep', '--f0-estimator-path', default="f0_estimator.pt")
    parser.add_argument('-k', default=4, type=int)
    parser.add_argument('-c', '--chunk', default=48000, type=int)
    parser.add_argument('--window-batch', default=64, type=int, help="windows per device batch")
    parser.add_argument('--no-trim-context', action='store_true',
                        help="run the kNN match and the decoder over all three chunks of every window (same samples)")
    parser.add_argument('--auto-pitch', action='store_true',
                        help="jobs follow their target voice's register unless their \"auto_pitch\" says otherwise")
    parser.add_argument('--auto-range', action='store_true',
                        help="jobs match their target voice's pitch range unless their \"auto_range\" says otherwise")
    parser.add_argument('-lim', '--limit', default=None, type=float, metavar="DB",
                        help="output limiter: no output sample exceeds this ceiling in dBFS (<= 0), so the 16-bit edge never wraps; the "
                             "gain starts to fall --limit-lookahead before a peak unless a job's \"limit_db\" says otherwise (default: no limiter)")
    parser.add_argument('--limit-lookahead', default=5.0, type=float, metavar="MS",
                        help="milliseconds over which the limiter's gain falls ahead of a peak and recovers after the hold (default 5)")
    parser.add_argument('--limit-hold', default=20.0, type=float, metavar="MS",
                        help="milliseconds the limiter's gain stays down after a peak (default 20)")
    parser.add_argument('-lufs', '--lufs', default=None, type=float, metavar="L",
                        help="loudness normalisation: every output file is brought to this integrated loudness in LUFS (ITU-R BS.1770-4, "
                             "-70 < L <= 0, e.g. -23 or -16) by one gain unless a job's \"lufs\" says otherwise, after the gain and before "
                             "the limiter and \"normalize\" (default: the level is left alone)")
    parser.add_argument('--loudness-max-db', default=12.0, type=float, metavar="DB",
                        help="the most the loudness normalisation turns a file up or down (default 12)")
    parser.add_argument('-env', '--envelope', default=0.0, type=float, metavar="A",
                        help="envelope follow: the converted voices take on their sources' loudness contours by this amount, 0 (off, the "
                             "default) to 1, unless a job's \"envelope\" says otherwise (module/multistream.py follow_envelope).  It can lift samples above full "
                             "scale: use -lim beside it")
    parser.add_argument('--envelope-floor', default=-60.0, type=float, metavar="DB",
                        help="the level under which the envelope follow stops telling the two signals apart (default -60)")
    parser.add_argument('--envelope-range', default=12.0, type=float, metavar="DB",
                        help="the most the envelope follow turns a frame up or down (default 12)")
    parser.add_argument('--envelope-radius', default=1, type=int, metavar="FRAMES",
                        help="20 ms frames on each side over which the envelope follow smooths both levels, 0 to 4 (default 1: 60 ms)")
    parser.add_argument('-pf', '--post-filter-alpha', default=0.0, type=float, metavar="A",
                        help="adaptive formant post filter on the converted waves at 16 kHz, ahead of -env: the alpha of the denominator, "
                             "0 (off, the default) to 0.85, unless a job's \"post_filter\" says otherwise (module/multistream.py post_filter)")
    parser.add_argument('--post-filter-ratio', default=0.625, type=float, metavar="R",
                        help="the post filter's numerator alpha as a share of the denominator's, 0 to 1 (default 0.625)")
    parser.add_argument('--post-filter-tilt', default=0.5, type=float, metavar="T",
                        help="the share of the post filter's spectral tilt that is taken out again, 0 to 1 (default 0.5)")
    parser.add_argument('--pcm16', action='store_true', help="write 16-bit PCM instead of float32 WAV")
    common.add_track_arguments(parser)      # (-pt: jobs track unless their "pitch_track" says otherwise)
    common.add_voicing_arguments(parser)    # (-vd: jobs decide unless their "voicing" says otherwise)
    common.add_path_arguments(parser)       # (-mp: jobs take the match path unless their "match_path" says otherwise)
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
    """an entry's "range_st" (None without one): a number of semitones > 0, for a voice given by "lib" alone, beside "register_hz"""
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


def declared_ranges(jobs):
    """{voice key: semitones} of the jobs' "range_st"; ValueError if two jobs declare different ones for one voice"""
    out = {}
    for i, j in enumerate(jobs):
        if j.get("range_st") is not None:
            key = voice_key(j)
            if out.setdefault(key, j["range_st"]) != j["range_st"]:
                raise ValueError(f"job {i}: \"range_st\" {j['range_st']} but an earlier job gave this voice {out[key]}")
    return out


def declared_registers(jobs):
    """{voice key: Hz} of the jobs' "register_hz"; ValueError if two jobs declare different ones for one voice"""
    out = {}
    for i, j in enumerate(jobs):
        if j.get("register_hz") is not None:
            key = voice_key(j)
            if out.setdefault(key, j["register_hz"]) != j["register_hz"]:
                raise ValueError(f"job {i}: \"register_hz\" {j['register_hz']} but an earlier job gave this voice {out[key]}")
    return out


def job_limit(j, where, limit_db=None, lookahead_ms=5.0, hold_ms=20.0):
    """an entry's "limit_db" (default `limit_db`; a JSON null switches the default off) -> a float <= 0, or None for a job without a
    limiter; ValueError otherwise (the two times are those of the flags, checked with it)"""
    from module.multistream import check_limit
    db = j.get("limit_db", limit_db)
    try:
        check_limit(db, lookahead_ms, hold_ms)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return None if db is None else float(db)


def job_loudness(j, where, lufs=None, max_db=12.0):
    """an entry's "lufs" (default `lufs`; a JSON null switches the default off) -> a float in (-70, 0], or None for a job whose level
    is left alone; ValueError otherwise (the largest gain is the flag's, checked with it)"""
    from module.multistream import check_loudness
    target = j.get("lufs", lufs)
    try:
        check_loudness(target, max_db)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return None if target is None else float(target)


def job_envelope(j, where, envelope=0.0, floor_db=-60.0, range_db=12.0, radius=1):
    """an entry's "envelope" (default `envelope`; a JSON null or 0 switches the default off) -> the amount as a float in (0, 1], or
    None for a job that does not follow; ValueError otherwise (the three tuning values are those of the flags, checked with it)"""
    from module.multistream import check_envelope
    a = j.get("envelope", envelope)
    try:
        a = check_envelope(0.0 if a is None else a, floor_db, range_db, radius)[0]
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return a if a > 0 else None


def job_post_filter(j, where, alpha=0.0, ratio=0.625, tilt=0.5):
    """an entry's "post_filter" (default `alpha`; a JSON null or 0 switches the default off) -> the alpha as a float in (0, 0.85], or
    None for a job that is not filtered; ValueError otherwise (ratio and tilt are those of the flags, checked with it)"""
    from module.multistream import check_post_filter
    a = j.get("post_filter", alpha)
    try:
        a = check_post_filter(0.0 if a is None else a, ratio, tilt)[0]
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return a if a > 0 else None


def job_track(j, where, pitch_track=False, weight=common.TRACK_WEIGHT, jump=common.TRACK_JUMP):
    """an entry's "pitch_track" (default `pitch_track`): true, false or {"weight": W, "jump": J} (defaults `weight`, `jump`) ->
    {"weight": W, "jump": J} as floats, or None for a job that does not track; ValueError otherwise, and together with
    "world_pitch" """
    v = j.get("pitch_track", bool(pitch_track))
    try:
        base = dict(weight=common.track_param("weight", weight), jump=common.track_param("jump", jump))
        if isinstance(v, dict):
            unknown = set(v) - {"weight", "jump"}
            if unknown:
                raise ValueError(f"\"pitch_track\": unknown keys {sorted(unknown)} (weight, jump; lo, hi and band are flags of the run)")
            base.update({key: common.track_param(key, val) for key, val in v.items()})
        elif not isinstance(v, bool):
            raise ValueError(f"\"pitch_track\" must be true, false or an object with weight / jump, got {v!r}")
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    if v is False:
        return None
    if j.get("world_pitch", False):
        raise ValueError(f"{where}: \"pitch_track\" cannot be combined with \"world_pitch\"")
    return base


def job_path(j, where, match_path=False, weight=common.PATH_WEIGHT):
    """an entry's "match_path" (default `match_path`): true, false or {"weight": W} (default `weight`) -> {"weight": W} as a float, or
    None for a job whose match takes no path; ValueError otherwise"""
    v = j.get("match_path", bool(match_path))
    try:
        base = dict(weight=common.path_param(weight))
        if isinstance(v, dict):
            base = common.path_options(dict(base, **v), "\"match_path\"")
        elif not isinstance(v, bool):
            raise ValueError(f"\"match_path\" must be true, false or an object with weight, got {v!r}")
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return None if v is False else base


def job_voicing(j, where, voicing=False, on=common.VOICING_ON, off=common.VOICING_OFF, floor_db=common.VOICING_FLOOR_DB):
    """an entry's "voicing" (default `voicing`): true, false or {"on": R, "off": R, "floor_db": DB} (defaults `on`, `off`, `floor_db`)
    -> {"on": R, "off": R, "floor_db": DB} as floats, or None for a job that does not decide; ValueError otherwise, and together with
    "world_pitch" """
    v = j.get("voicing", bool(voicing))
    base = dict(on=on, off=off, floor_db=floor_db)
    if isinstance(v, dict):
        unknown = set(v) - set(base)
        if unknown:
            raise ValueError(f"{where}: \"voicing\": unknown keys {sorted(unknown)} (on, off, floor_db; lo and hi are flags of the run)")
        base.update(v)
    elif not isinstance(v, bool):
        raise ValueError(f"{where}: \"voicing\" must be true, false or an object with on / off / floor_db, got {v!r}")
    o = common.voicing_options(base, where)
    if v is False:
        return None
    if j.get("world_pitch", False):
        raise ValueError(f"{where}: \"voicing\" cannot be combined with \"world_pitch\"")
    return {key: o[key] for key in ("on", "off", "floor_db")}


def load_jobs(path, k=4, auto_pitch=False, limit_db=None, lookahead_ms=5.0, hold_ms=20.0, envelope=0.0, envelope_floor_db=-60.0,
              envelope_range_db=12.0, envelope_radius=1, auto_range=False, pitch_track=False, track_weight=common.TRACK_WEIGHT,
              track_jump=common.TRACK_JUMP, lufs=None, loudness_max_db=12.0, voicing=False, voicing_on=common.VOICING_ON,
              voicing_off=common.VOICING_OFF, voicing_floor_db=common.VOICING_FLOOR_DB, match_path=False,
              path_weight=common.PATH_WEIGHT, post_filter=0.0, post_filter_ratio=0.625, post_filter_tilt=0.5):
    """the jobs file -> list of dicts with every key filled in (paths relative to the file's folder; "auto_pitch": default
    `auto_pitch`); a limited job ("limit_db", default `limit_db`) also carries "limit_db", a job without a limiter does not, so a
    file without the key loads to what it did; likewise "envelope" (default `envelope`) only on a job that follows at an amount above
    0, "auto_range" (default `auto_range`) only on a job that is on, "range_st" only where the entry has it and "pitch_track"
    (default `pitch_track` at `track_weight` / `track_jump`) only on a job that tracks and "lufs" (default `lufs`) only on a job that
    is normalised and "voicing" (default `voicing` at `voicing_on` / `voicing_off` / `voicing_floor_db`) only on a job that decides and
    "match_path" (default `match_path` at `path_weight`) only on a job whose match takes a path and "post_filter" (default
    `post_filter`) only on a job that is filtered at an alpha above 0;
    ValueError on a malformed job, before anything runs on the device"""
    job_voicing({}, "-vd / --voicing-on / --voicing-off / --voicing-floor", voicing, voicing_on, voicing_off, voicing_floor_db)
    job_track({}, "-pt / --track-weight / --track-jump", pitch_track, track_weight, track_jump)
    job_path({}, "-mp / --path-weight", match_path, path_weight)
    job_limit({}, "-lim / --limit-lookahead / --limit-hold", limit_db, lookahead_ms, hold_ms)
    job_loudness({}, "-lufs / --loudness-max-db", lufs, loudness_max_db)
    env = (envelope_floor_db, envelope_range_db, envelope_radius)
    job_envelope({}, "-env / --envelope-floor / --envelope-range / --envelope-radius", envelope, *env)
    job_post_filter({}, "-pf / --post-filter-ratio / --post-filter-tilt", post_filter, post_filter_ratio, post_filter_tilt)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k={k} outside [1, {MAX_K}] (the pool search's limit)")
    with open(path) as f:
        jobs = json.load(f)
    if not isinstance(jobs, list) or not jobs:
        raise ValueError(f"{path}: expected a non-empty JSON list of jobs")
    base = os.path.dirname(os.path.abspath(path))
    rel = lambda p: None if p is None else (p if os.path.isabs(p) else os.path.join(base, p))      # noqa: E731
    out = []
    for i, j in enumerate(jobs):
        if not isinstance(j, dict) or "input" not in j:
            raise ValueError(f"job {i}: an object with an \"input\" wav is required")
        unknown = (set(j) - set(JOB_KEYS) - set(LIMIT_KEYS) - set(ENVELOPE_KEYS) - set(RANGE_KEYS) - set(TRACK_KEYS)
                   - set(LOUDNESS_KEYS) - set(VOICING_KEYS) - set(PATH_KEYS) - set(POSTFILTER_KEYS))
        if unknown:
            raise ValueError(f"job {i}: unknown keys {sorted(unknown)} (known: "
                             f"{JOB_KEYS + LIMIT_KEYS + ENVELOPE_KEYS + RANGE_KEYS + TRACK_KEYS + LOUDNESS_KEYS + VOICING_KEYS + PATH_KEYS + POSTFILTER_KEYS})")
        blend = blend_sources(j, f"job {i}", rel) if "blend" in j else None
        if blend is None and j.get("target") is None and j.get("lib") is None:
            raise ValueError(f"job {i}: needs a \"target\" wav and / or a \"lib\" voice library")
        if not isinstance(j.get("world_pitch", False), bool):
            raise ValueError(f"job {i}: \"world_pitch\" must be true or false, got {j['world_pitch']!r}")
        if not isinstance(j.get("auto_pitch", False), bool):
            raise ValueError(f"job {i}: \"auto_pitch\" must be true or false, got {j['auto_pitch']!r}")
        if not isinstance(j.get("auto_range", False), bool):
            raise ValueError(f"job {i}: \"auto_range\" must be true or false, got {j['auto_range']!r}")
        job_k = check_k(j["k"], f"job {i}: \"k\"") if "k" in j else k
        e = dict(input=rel(j["input"]), target=rel(j.get("target")), lib=rel(j.get("lib")), output=rel(j.get("output")),
                 pitch=float(j.get("pitch", 0.0)), intonation=float(j.get("intonation", 1.0)), f0_rate=float(j.get("f0_rate", 1.0)),
                 alpha=float(j.get("alpha", 0.0)), gain=float(j.get("gain", 1.0)), normalize=bool(j.get("normalize", False)),
                 world_pitch=j.get("world_pitch", False), blend=blend, k=job_k,
                 auto_pitch=j.get("auto_pitch", bool(auto_pitch)), register_hz=register_hz_of(j, f"job {i}"))
        lim = job_limit(j, f"job {i}", limit_db, lookahead_ms, hold_ms)
        if lim is not None:
            e["limit_db"] = lim
        target = job_loudness(j, f"job {i}", lufs, loudness_max_db)
        if target is not None:
            e["lufs"] = target
        amount = job_envelope(j, f"job {i}", envelope, *env)
        if amount is not None:
            e["envelope"] = amount
        pfa = job_post_filter(j, f"job {i}", post_filter, post_filter_ratio, post_filter_tilt)
        if pfa is not None:
            e["post_filter"] = pfa
        if j.get("auto_range", bool(auto_range)):
            e["auto_range"] = True
        track = job_track(j, f"job {i}", pitch_track, track_weight, track_jump)
        if track is not None:
            e["pitch_track"] = track
        decide = job_voicing(j, f"job {i}", voicing, voicing_on, voicing_off, voicing_floor_db)
        if decide is not None:
            e["voicing"] = decide
        path_ = job_path(j, f"job {i}", match_path, path_weight)
        if path_ is not None:
            e["match_path"] = path_
        range_st = range_st_of(j, f"job {i}")
        if range_st is not None:
            e["range_st"] = range_st
        for key in ("input", "target", "lib"):
            if e[key] is not None and not os.path.isfile(e[key]):
                raise ValueError(f"job {i}: {key} {e[key]!r} does not exist")
        for c, (tgt, lib, _) in enumerate(blend or ()):
            for key, f in (("target", tgt), ("lib", lib)):
                if f is not None and not os.path.isfile(f):
                    raise ValueError(f"job {i}: blend component {c}: {key} {f!r} does not exist")
        out.append(e)
    return out


def voice_key(job):
    """jobs (and blend components: (target, lib, weight)) with the same voice sources share one pool voice"""
    if isinstance(job, tuple):
        return (job[0], job[1])
    return (job["target"], job["lib"])


def voice_keys(job):
    """the voice sources a job needs: its own, or those of its blend's components"""
    return [voice_key(c) for c in job["blend"]] if job.get("blend") else [voice_key(job)]


def job_voice(job, names):
    """the job's voice for Converter.convert_many: a pool name, or (name, weight) pairs for a blend"""
    if job.get("blend"):
        return [(names[voice_key(c)], c[2]) for c in job["blend"]]
    return names[voice_key(job)]


def check_voice_sizes(sizes, k):
    """sizes: voice key -> vectors; ValueError for a voice shorter than k"""
    for key, m in sizes.items():
        if m < k:
            raise ValueError(f"voice {key}: {m} vectors, fewer than k={k}")


def check_job_voice_sizes(jobs, sizes):
    """every voice a job uses (blend components included) against the job's own k"""
    for job in jobs:
        check_voice_sizes({key: sizes[key] for key in voice_keys(job)}, job["k"])


def jobs_k(jobs, k):
    """convert_many's k: the scalar -k when every job runs at it (the uniform path, as before), else the per-job list"""
    ks = [job["k"] for job in jobs]
    return k if all(v == k for v in ks) else ks


def main(argv=None):
    args = build_parser().parse_args(argv)
    device = torch.device(args.device)
    if device.type != "cuda":
        raise SystemExit("this build runs on the MI355X only: pass -d cuda")
    try:
        tw, tj, lo, hi, band = common.track_arguments(args)             # (before anything is loaded)
        common.voicing_arguments(args)                                  # (likewise: --voicing-lo / --voicing-hi and the defaults)
        common.path_arguments(args)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    jobs = load_jobs(args.jobs, args.k, args.auto_pitch, args.limit, args.limit_lookahead, args.limit_hold, args.envelope,
                     args.envelope_floor, args.envelope_range, args.envelope_radius, args.auto_range, args.pitch_track, tw, tj,
                     args.lufs, args.loudness_max_db, args.voicing, args.voicing_on, args.voicing_off, args.voicing_floor,
                     args.match_path, args.path_weight, args.post_filter_alpha, args.post_filter_ratio, args.post_filter_tilt)
    pathed = any("match_path" in j for j in jobs)
    tracked = any("pitch_track" in j for j in jobs)
    deciding = any("voicing" in j for j in jobs)
    on_auto = any(j["auto_pitch"] for j in jobs)
    ranged = any("auto_range" in j for j in jobs)
    auto = on_auto or ranged                            # only then are the voices' registers (and ranges) measured or declared
    declared = declared_registers(jobs) if auto else {}
    declared_st = declared_ranges(jobs) if ranged else {}
    # (device work starts here)
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    from module.multistream import (VoicePool, follow_envelope, limit_waves, measure_register, normalize_loudness, pitch_hz,
                                    post_filter)
    from module.pipeline import Converter
    from module.spectrogram import spectrogram
    from module.voice_library import VoiceLibrary

    PE, CE, Dec = F0Estimator().to(device), ContentEncoder().to(device), Decoder().to(device)
    PE.load_state_dict(torch.load(args.f0_estimator_path, map_location=device))
    CE.load_state_dict(torch.load(args.content_encoder_path, map_location=device))
    Dec.load_state_dict(torch.load(args.decoder_path, map_location=device))
    os.makedirs(args.outputs, exist_ok=True)

    voices, registers = {}, {}
    for key in (key for job in jobs for key in voice_keys(job)):        # inference.py:86-92 per distinct voice
        if key in voices:
            continue
        target, lib = key
        tgt = torch.zeros(1, 768, 0, device=device)
        if target is not None:
            wf, sr = audio_io.load(target)
            wf = audio_io.resample(wf.to(device), sr, 16000)
            wf = wf / wf.abs().max()
            tgt = CE(spectrogram(wf[:1]))
            if auto:                                                    # the voice's register, on the audio the encoder saw
                registers[key] = measure_register(PE, wf[:1].contiguous())
        if lib is not None:
            VL = VoiceLibrary().to(device)
            VL.load_state_dict(torch.load(lib, map_location=device))
            tgt = torch.cat([tgt, VL.tokens], dim=2)
        voices[key] = tgt
        if key in declared:
            p0 = pitch_hz(declared[key])
            registers[key] = (p0, 1.0) if key not in declared_st else (p0, 1.0, p0 * p0 + declared_st[key] * declared_st[key])
    check_job_voice_sizes(jobs, {k_: int(t.shape[2]) for k_, t in voices.items()})
    names = {key: f"voice{i}" for i, key in enumerate(voices)}
    pool = VoicePool({names[key]: t for key, t in voices.items()}, device=device,
                     registers={names[key]: r for key, r in registers.items()})
    print(f"{len(jobs)} jobs over {len(voices)} voices ({pool.P} vectors)")

    utts, rates = [], []
    for job in jobs:
        wf, sr = audio_io.load(job["input"])
        wf = audio_io.resample(wf.to(device), sr, 16000)
        wf = wf / wf.abs().max()
        utts.append(wf.mean(dim=0, keepdim=True))
        rates.append(sr)
    conv = Converter(CE, PE, Dec, device)
    outs = conv.convert_many(utts, pool, [job_voice(j, names) for j in jobs], pitch_shift=[j["pitch"] for j in jobs],
                             intonation=[j["intonation"] for j in jobs], f0_rate=[j["f0_rate"] for j in jobs],
                             alpha=[j["alpha"] for j in jobs], world_pitch=[j["world_pitch"] for j in jobs],
                             auto_pitch=[j["auto_pitch"] for j in jobs] if on_auto else False,
                             **(dict(auto_range=["auto_range" in j for j in jobs]) if ranged else {}),
                             **(dict(pitch_track=[dict(j["pitch_track"], lo=lo, hi=hi, band=band) if "pitch_track" in j else None
                                                  for j in jobs]) if tracked else {}),
                             **(dict(voicing=[dict(j["voicing"], lo=args.voicing_lo, hi=args.voicing_hi) if "voicing" in j else None
                                              for j in jobs]) if deciding else {}),
                             **(dict(match_path=[j.get("match_path") for j in jobs]) if pathed else {}), chunk=args.chunk, k=jobs_k(jobs, args.k), window_batch=args.window_batch,
                             trim_context=not args.no_trim_context)
    for i, (job, out, sr) in enumerate(zip(jobs, outs, rates)):
        if job.get("post_filter"):                                      # at 16 kHz, first: the envelope sets the level of the filtered wave
            out = post_filter(out, None, job["post_filter"], args.post_filter_ratio, args.post_filter_tilt)
        if job.get("envelope"):                                         # at 16 kHz, against the source the converter saw
            out = follow_envelope(out, utts[i], None, job["envelope"], args.envelope_floor, args.envelope_range, args.envelope_radius)
        out = audio_io.resample(out, 16000, sr, post_gain_db=job["gain"])
        if job.get("lufs") is not None:                                 # on the device, at the file's own rate, ahead of the limiter
            out = normalize_loudness(out, None, job["lufs"], int(sr), args.loudness_max_db)
        if job.get("limit_db") is not None:                             # on the device, before the normalisation and the save
            out = limit_waves(out, None, job["limit_db"], args.limit_lookahead, args.limit_hold, sr)
        out = out.cpu()
        if job["normalize"]:
            out = out / out.abs().max()
        path = job["output"] or os.path.join(args.outputs, f"{i}_{os.path.splitext(os.path.basename(job['input']))[0]}.wav")
        audio_io.save(path, out, sr, "pcm16" if args.pcm16 else "float32")
        print(f"-> {path}")


if __name__ == "__main__":
    main()
