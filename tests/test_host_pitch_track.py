"""CPU tests of pitch tracking: the NumPy restatement tools/pitch_track_ref.py (against a brute-force enumeration of every path, the
three cases the tracker is for -- octave outliers, a real step, a glide -- and its identities), the tables the host builds, the C ABI
(symbols, prototypes, SRCS, the refusals that need no device), every refusal of the converters' host logic, the sessions / jobs files
and the flags of the four CLIs."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import batch_inference as BI                                         # noqa: E402
import multistream_inference as MSI                                  # noqa: E402
import pitch_track_ref as PR                                         # noqa: E402
from module import _native as nat                                    # noqa: E402
from module import common                                            # noqa: E402
from module import multistream as MS                                 # noqa: E402

T = 33


@pytest.fixture(scope="module")
def tracker():
    return PR.Tracker()                                              # 50 .. 1100 Hz, a band of 2 semitones


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("band,weight,jump", [(0.2, 1.0, 0.5), (0.4, 3.0, 1.0), (1.0, 0.0, 0.0)])
def test_the_recurrence_finds_the_best_of_all_paths(band, weight, jump):
    """5 states x 5 frames: all 3125 paths enumerated.  At 100 .. 104 Hz neighbouring classes lie 0.17 semitones apart, so the three
    bands hold 1, 2 and every neighbour on each side"""
    tr = PR.Tracker(100, 104, band)
    assert [int(b - a) for a, b in zip(tr.blo, tr.bhi)][2] == {0.2: 2, 0.4: 4, 1.0: 4}[band]
    for seed in range(4):
        x = np.random.default_rng(seed).standard_normal((4096, 5)).astype(np.float32)
        best, score, ties = PR.brute_force(x, tr, weight, jump)
        if weight == jump == 0:                                      # every move is free: the argmax of each frame, whatever led to it
            assert np.array_equal(tr.path(x, weight, jump), x[100:105].argmax(axis=0))
        else:
            assert ties == 1 and np.array_equal(tr.path(x, weight, jump), best), seed


def test_octave_outliers_are_smoothed_away(tracker):
    odd = (5, 17, 18)
    x = PR.ridge_scores([[200, 400] if t in odd else [200] for t in range(T)], [[8, 14] if t in odd else [10] for t in range(T)])
    plain = x.argmax(axis=0)
    assert all(399 <= plain[t] <= 401 for t in odd) and all(199 <= plain[t] <= 201 for t in range(T) if t not in odd)
    f0 = tracker.track(x)
    assert f0.dtype == np.float32 and f0.min() >= 199 and f0.max() <= 201


def test_a_real_step_is_followed_at_its_frame(tracker):
    x = PR.ridge_scores([[120] if t < 16 else [240] for t in range(T)], [[10]] * T)
    f0 = tracker.track(x)
    assert np.all(np.abs(f0[:16] - 120) <= 2) and np.all(np.abs(f0[16:] - 240) <= 2)


def test_a_glide_is_followed(tracker):
    centres = [150 + 40 * t / (T - 1) for t in range(T)]
    f0 = tracker.track(PR.ridge_scores([[c] for c in centres], [[10]] * T))
    assert np.abs(f0 - np.array(centres)).max() <= 2


def test_the_identities(tracker):
    x = np.random.default_rng(3).standard_normal((4096, 9)).astype(np.float32)
    inside = x[50:1101].argmax(axis=0).astype(np.float32) + 50
    assert tracker.track(x[:, :1])[0] == inside[0]                   # one frame: the argmax over [lo, hi]
    assert np.array_equal(tracker.track(x, 0.0, 0.0), inside)       # free moves: the per-frame argmax over [lo, hi]
    tie = x.copy()
    tie[61] = tie[60] = 50.0                                         # ... the lowest class on ties
    assert np.all(tracker.track(tie, 0.0, 0.0) == 60)
    flat = np.full((4096, 7), 0.25, dtype=np.float32)
    for w, k in ((1.0, 12.0), (0.0, 0.0), (3.0, 0.5)):               # all-equal scores: the lowest class everywhere
        assert np.all(tracker.track(flat, w, k) == 50)
    assert tracker.track(x).min() >= 50                              # class 0 is not a state
    e = PR.scores(np.array([[np.nan, np.inf, -np.inf, 1.5]] * 3, dtype=np.float32).T.copy(), 0, 4)
    assert e.dtype == np.float64 and e.shape == (3, 4) and e[0].tolist() == [-PR.FLT_MAX, PR.FLT_MAX, -PR.FLT_MAX, 1.5]


def test_an_all_nan_frame_leaves_the_neighbours_classes_on_the_ridge(tracker):
    """A ridge at 300 Hz (h = 10) over 9 frames with frame 4 all NaN.  Every score of that frame is -FLT_MAX = -3.4e38, whose spacing in
    fp64 is 2^75 = 3.8e22: D[4][i] = -FLT_MAX + m would round every m (about 40 here) away, all states would tie from that frame on
    and frames 4 .. 8 would decode to 50, the lowest class.  The scores of a frame are taken relative to the frame's best one, so
    the frame is e = 0 and the path crosses it on the ridge.  The same for an all -inf frame, and a +inf entry pins its own frame only"""
    ridge = PR.ridge_scores([[300]] * 9, [[10]] * 9)
    for bad in (np.nan, -np.inf, np.inf):
        x = ridge.copy()
        x[:, 4] = bad
        f0 = tracker.track(x)
        print("tracked classes:", f0.tolist())
        assert np.all(np.abs(f0 - 300) <= 2)
    x = ridge.copy()
    x[700, 4] = np.inf
    f0 = tracker.track(x)
    assert f0[4] == 700 and np.all(np.abs(np.delete(f0, 4) - 300) <= 2)


def test_track_rows_leaves_rows_that_are_off_and_counts_the_frames_it_moves(tracker):
    x = np.random.default_rng(4).standard_normal((3, 4096, 6)).astype(np.float32)
    before = np.full((3, 6), 77.0, dtype=np.float32)
    before[2] = tracker.track(x[2], 3.0, 0.5)
    before[2, 1] += 1
    out, changed = PR.track_rows(x, before, tracker, [1, 0, 1], [1.0, 0.0, 3.0], [12.0, 0.0, 0.5])
    assert np.array_equal(out[1], before[1]) and np.array_equal(out[0], tracker.track(x[0])) and changed.tolist()[1:] == [0, 1]
    assert changed[0] == int((out[0] != 77).sum())


# ------------------------------------------------------------------------------------------------ the host's tables and checks
def test_the_hosts_tables_are_the_restatements(tracker):
    for lo, hi, band in ((50, 1100, 2.0), (77, 77, 2.0), (96, 4095, 0.5), (1, 40, 0.0)):
        s, blo, bhi = common.pitch_track_tables(lo, hi, band)
        rs, rlo, rhi = PR.tables(lo, hi, band)
        assert np.array_equal(s.view(np.int64), rs.view(np.int64)) and np.array_equal(blo, rlo) and np.array_equal(bhi, rhi)
        assert s.dtype == np.float64 and blo.dtype == bhi.dtype == np.int32 and len(s) == hi - lo + 1
        i = np.arange(len(s))
        assert np.all(blo <= i) and np.all(i <= bhi)
        for k in (0, len(s) // 2, len(s) - 1):                       # the first and the last state within the band, exactly
            near = np.flatnonzero(np.abs(s[k] - s) <= band)
            assert (blo[k], bhi[k]) == (near[0], near[-1])
    assert (common.TRACK_LO, common.TRACK_HI, common.TRACK_BAND, common.TRACK_WEIGHT, common.TRACK_JUMP) == \
        (PR.LO, PR.HI, PR.BAND, PR.WEIGHT, PR.JUMP) == (50, 1100, 2.0, 1.0, 12.0)
    assert common.TRACK_MAX_STATES == PR.MAX_STATES == 4000
    t = common.pitch_track(60, 90, 1.0, "cpu")                       # (the tables as tensors; nothing of it touches a device)
    assert (t.lo, t.hi, t.band, t.states) == (60, 90, 1.0, 31) and t.semis.dtype == torch.float64 and t.band_lo.dtype == torch.int32


def test_bad_ranges_bands_and_weights_are_refused():
    for lo, hi in ((0, 100), (-1, 5), (200, 100), (50, 4096), (1.5, 100), (True, 100)):
        with pytest.raises(ValueError, match="pitch track: "):
            common.pitch_track_tables(lo, hi, 2.0)
    with pytest.raises(ValueError, match="4001 states, at most 4000"):
        common.pitch_track_tables(95, 4095, 2.0)
    with pytest.raises(ValueError, match="4095 states, at most 4000"):
        common.pitch_track(1, 4095, 2.0, "cuda")                     # (refused before the device is touched)
    for band in (-0.1, float("nan"), float("inf"), "2", True, None):
        with pytest.raises(ValueError, match="band must be a finite number of semitones >= 0"):
            common.pitch_track_tables(50, 1100, band)
    for bad in (-1, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="weight must be a finite number >= 0"):
            common.track_param("weight", bad)
    assert common.track_param("jump", 3) == 3.0 and isinstance(common.track_param("jump", 3), float)
    assert common.track_options(None) is None and common.track_options(False) is None
    assert common.track_options(True) == dict(weight=1.0, jump=12.0, lo=50, hi=1100, band=2.0)
    assert common.track_options({"weight": 3}) == dict(weight=3.0, jump=12.0, lo=50, hi=1100, band=2.0)
    for bad, msg in ((1, "expected None, a bool or a dict"), ({"width": 2}, r"unknown keys \['width'\]"), ({"jump": -2}, "jump must be")):
        with pytest.raises(ValueError, match=msg):
            common.track_options(bad)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_symbols_are_exported_and_the_prototypes_agree_with_the_header():
    L = ctypes.CDLL(nat.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    for name, res, nargs in (("alive_f0_track_rows", ctypes.c_int, 16), ("alive_f0_logits", ctypes.c_int, 7),
                             ("alive_f0_track_workspace_bytes", ctypes.c_size_t, 3)):
        assert hasattr(L, name)
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl is not None, f"{name} is not declared in alive_vc.h"
        args = decl.group(1).split(",")
        assert len(args) == nargs == len(nat.PROTOTYPES[name][1]) and nat.PROTOTYPES[name][0] is res
        assert [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args] == nat.PROTOTYPES[name][1], name
    assert re.search(r"#define\s+ALIVE_F0_TRACK_MAX_STATES\s+4000\b", hdr)
    mk = open(os.path.join(ROOT, "alive-vc_amd", "csrc", "Makefile")).read()
    assert "f0_track.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]
    assert "-ffp-contract=off" in mk and "-fno-fast-math" in mk


def test_the_abi_refuses_bad_arguments_without_a_device():
    L = nat.lib()
    #     logits N  C     T  lo  S     semis band_lo band_hi on    weight jump f0    changed ws     stream
    ok = [4096,  2, 4096, 5, 50, 1051, 8192, 16384,  32768,  None, 65536, 65536, 131072, None, 262144, None]
    for change, msg in (({5: 4001}, b"states"), ({5: 0}, b"states"), ({4: 0}, b"lo < 1"), ({4: 3046}, b"outside"), ({2: 1100}, b"outside"),
                        ({3: 0}, b"T < 1"), ({6: None}, b"null tables"), ({7: None}, b"null tables"), ({8: None}, b"null tables"),
                        ({0: None}, b"null pointer"), ({10: None}, b"null pointer"), ({12: None}, b"null pointer"),
                        ({14: None}, b"null pointer"), ({1: 0}, b"N outside")):
        a = list(ok)
        for i, v in change.items():
            a[i] = v
        assert L.alive_f0_track_rows(*a) == -1 and msg in L.alive_last_error(), change
    assert L.alive_f0_track_workspace_bytes(3, 7, 31) >= 3 * 7 * 31 * 2
    assert L.alive_f0_track_workspace_bytes(128, 24, 1051) >= 128 * 24 * 1051 * 2
    assert L.alive_f0_track_workspace_bytes(0, 7, 31) == L.alive_f0_track_workspace_bytes(3, 0, 31) == 0
    assert L.alive_f0_logits(None, 4096, 1, 5, 8192, 16384, None) == -1 and b"alive_f0_logits" in L.alive_last_error()


# ------------------------------------------------------------------------------------------------ the converters' host logic
def _host_converter(pitch_track):
    """the part of a converter the tracker's validation reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.pitch_track = pitch_track
    return c


def test_session_settings_are_checked_against_the_converter():
    assert {"pitch_track", "track_weight", "track_jump"} <= set(MS._PARAMS)
    on, off = _host_converter(True), _host_converter(False)
    assert on._session_track(0, dict(pitch_track=True, track_weight=2, track_jump=0)) == (1, 2.0, 0.0)
    assert on._session_track(0, {}) == (0, 1.0, 12.0) == off._session_track(0, dict(pitch_track=False))
    with pytest.raises(ValueError, match=r"slot 2: pitch_track=True needs a converter built with MultiStreamConverter\(..., pitch_track=True\)"):
        off._session_track(2, dict(pitch_track=True))
    with pytest.raises(ValueError, match="slot 1: pitch_track cannot be combined with world_pitch"):
        on._session_track(1, dict(pitch_track=True, world_pitch=True))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="slot 1: pitch_track must be a bool"):
            on._session_track(1, dict(pitch_track=bad))
    for key in ("track_weight", "track_jump"):
        for bad in (-1, float("nan"), float("inf"), "1", True):
            for conv in (on, off):
                with pytest.raises(ValueError, match=f"slot 1: pitch track: {key} must be a finite number >= 0"):
                    conv._session_track(1, {key: bad})
    with pytest.raises(ValueError, match="pitch_track must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, pitch_track=1)
    with pytest.raises(ValueError, match="MultiStreamConverter: pitch track: 4001 states, at most 4000"):
        MS.MultiStreamConverter(None, None, None, None, 1, pitch_track=True, track_lo=95, track_hi=4095)
    with pytest.raises(ValueError, match="MultiStreamConverter: pitch track: needs 1 <= lo <= hi <= 4095"):
        MS.MultiStreamConverter(None, None, None, None, 1, pitch_track=True, track_lo=0)
    with pytest.raises(ValueError, match="MultiStreamConverter: pitch track: band must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, pitch_track=True, track_band=-1)
    with pytest.raises(ValueError, match=r"pitch_track_changed needs a converter built with MultiStreamConverter\(..., pitch_track=True\)"):
        off.pitch_track_changed()
    assert MS.MultiStreamConverter.pitch_track is False


def test_realtime_converter_checks_its_tracker_before_anything_is_built():
    from module.realtime import RealtimeConverter
    for bad, msg in ((1, "expected None, a bool or a dict"), ({"weight": -1}, "weight must be"), ({"lo": 0}, "needs 1 <= lo"),
                     ({"lo": 95, "hi": 4095}, "4001 states"), ({"band": float("nan")}, "band must be"), ({"x": 1}, "unknown keys")):
        with pytest.raises(ValueError, match=msg):
            RealtimeConverter(None, None, None, None, pitch_track=bad)
    with pytest.raises(ValueError, match="pitch_track cannot be combined with world_pitch"):
        RealtimeConverter(None, None, None, None, pitch_track=True, world_pitch=True)
    with pytest.raises(ValueError, match="interior reuse cannot be combined with pitch_track"):
        RealtimeConverter(None, None, None, None, pitch_track=True, reuse_interior=True)
    rt = RealtimeConverter.__new__(RealtimeConverter)
    assert rt.pitch_track is False
    with pytest.raises(ValueError, match="pitch_track_changed needs a converter built with"):
        rt.pitch_track_changed()


def test_the_offline_converter_refuses_world_with_track_and_bad_settings():
    from module.pipeline import Converter
    conv = Converter.__new__(Converter)
    conv.device = torch.device("cpu")
    win = torch.zeros(2, 9600)
    with pytest.raises(ValueError, match="pitch_track cannot be combined with world_pitch"):
        conv._convert_windows(win, world_pitch=True, pitch_track=True)
    with pytest.raises(ValueError, match="pitch_track cannot be combined with world_pitch"):
        conv.features(win, world_pitch=True, pitch_track=common.track_options(True))
    for bad, msg in (({"weight": -1}, "weight must be"), ({"hi": 5000}, "needs 1 <= lo <= hi <= 4095"), ({"lo": 95, "hi": 4095}, "4001 states"),
                     ("on", "expected None, a bool or a dict")):
        with pytest.raises(ValueError, match=msg):
            conv._convert_windows(win, pitch_track=bad)
    utts = [torch.zeros(1, 4000)] * 3
    with pytest.raises(ValueError, match="pitch_track: 2 values for 3 utterances"):
        conv.convert_many(utts, None, ["a", "b", "c"], pitch_track=[True, False])
    with pytest.raises(ValueError, match=r"convert_many: pitch_track\[2\]: unknown keys"):
        conv.convert_many(utts, None, ["a", "b", "c"], pitch_track=[True, False, {"width": 1}])
    with pytest.raises(ValueError, match="cannot be combined with world_pitch on the same utterance"):
        conv.convert_many(utts, None, ["a", "b", "c"], pitch_track=[True, False, False], world_pitch=[True, False, False])
    with pytest.raises(ValueError, match="lo, hi and band are call-wide"):
        conv.convert_many(utts, None, ["a", "b", "c"], pitch_track=[True, False, {"band": 1.0}])
    with pytest.raises(ValueError, match="cannot be combined with world_pitch"):
        MS.measure_register(None, torch.zeros(1, 3200), world_pitch=True, pitch_track=True)


# ------------------------------------------------------------------------------------------------ the files and the flags
@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "spk.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, entries, name="f.json"):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_sessions_file_takes_the_tracker_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    assert MSI.TRACK_KEYS == ("pitch_track", "track_weight", "track_jump")
    a, b, c, d = MSI.load_sessions(write(files, [sess, dict(sess, pitch_track=True), dict(sess, pitch_track=False, track_jump=3),
                                                 dict(sess, pitch_track=True, track_weight=2, track_jump=0)]))
    assert set(a) == set(MSI.SESSION_KEYS) == set(c)                 # a file without the keys parses to what it did
    assert set(b) == set(MSI.SESSION_KEYS) | set(MSI.TRACK_KEYS) == set(d)
    assert (b["pitch_track"], b["track_weight"], b["track_jump"]) == (True, 1.0, 12.0)
    assert (d["track_weight"], d["track_jump"]) == (2.0, 0.0) and isinstance(d["track_weight"], float)
    # -pt and its two values are the defaults; a session's false switches it off, its own values win
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, pitch_track=False), dict(sess, track_jump=1)]), pitch_track=True,
                                track_weight=0.5, track_jump=3.0)
    assert (a["track_weight"], a["track_jump"]) == (0.5, 3.0) and "pitch_track" not in b and (c["track_weight"], c["track_jump"]) == (0.5, 1.0)
    for bad in (1, "true", None, [True]):
        with pytest.raises(ValueError, match=r"session 1: \"pitch_track\" must be true or false"):
            MSI.load_sessions(write(files, [sess, dict(sess, pitch_track=bad)]))
    for bad in (-1, "1", True):
        with pytest.raises(ValueError, match=r"session 1: pitch track: \"track_weight\" must be"):
            MSI.load_sessions(write(files, [sess, dict(sess, track_weight=bad)]))
    with pytest.raises(ValueError, match=r"session 0: \"pitch_track\" cannot be combined with \"world_pitch\""):
        MSI.load_sessions(write(files, [dict(sess, pitch_track=True, world_pitch=True)]))
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['track_band'\]"):
        MSI.load_sessions(write(files, [dict(sess, track_band=2)]))
    with pytest.raises(ValueError, match=r"-pt / --track-weight / --track-jump: pitch track: \"track_jump\" must be"):
        MSI.load_sessions(write(files, [sess]), track_jump=-3)


def test_jobs_file_takes_the_tracker_per_job(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    assert BI.TRACK_KEYS == ("pitch_track",)
    a, b, c, d = BI.load_jobs(write(files, [job, dict(job, pitch_track=True), dict(job, pitch_track=False),
                                            dict(job, pitch_track={"weight": 3})]))
    assert set(a) == set(BI.JOB_KEYS) == set(c) and set(b) == set(BI.JOB_KEYS + BI.TRACK_KEYS) == set(d)
    assert b["pitch_track"] == dict(weight=1.0, jump=12.0) and d["pitch_track"] == dict(weight=3.0, jump=12.0)
    a, b, c = BI.load_jobs(write(files, [job, dict(job, pitch_track=False), dict(job, pitch_track={"jump": 1})]), pitch_track=True,
                           track_weight=0.5, track_jump=3.0)
    assert a["pitch_track"] == dict(weight=0.5, jump=3.0) and "pitch_track" not in b and c["pitch_track"] == dict(weight=0.5, jump=1.0)
    for bad in (1, "true", None, [True], {"lo": 60}, {"weight": -1}):
        with pytest.raises(ValueError, match=r"job 1: "):
            BI.load_jobs(write(files, [job, dict(job, pitch_track=bad)]))
    with pytest.raises(ValueError, match=r"job 0: \"pitch_track\" cannot be combined with \"world_pitch\""):
        BI.load_jobs(write(files, [dict(job, pitch_track=True, world_pitch=True)]))
    with pytest.raises(ValueError, match=r"job 0: unknown keys \['track_weight'\]"):
        BI.load_jobs(write(files, [dict(job, track_weight=2)]))
    with pytest.raises(ValueError, match=r"-pt / --track-weight / --track-jump: pitch track: weight must be"):
        BI.load_jobs(write(files, [job]), track_weight=float("nan"))


def test_all_four_clis_take_the_tracker_flags():
    import inference as INF
    import realtime_inference as RI
    for mod, argv in ((INF, []), (RI, []), (BI, ["j.json"]), (MSI, ["s.json"])):
        args = mod.build_parser().parse_args(argv)
        assert (args.pitch_track, args.track_weight, args.track_jump, args.track_lo, args.track_hi, args.track_band) == \
            (False, 1.0, 12.0, 50, 1100, 2.0)
        assert common.track_arguments(args) == (1.0, 12.0, 50, 1100, 2.0)
        args = mod.build_parser().parse_args(argv + ["-pt", "--track-weight", "0.5", "--track-jump", "3", "--track-lo", "60",
                                                     "--track-hi", "900", "--track-band", "1.5"])
        assert common.track_arguments(args) == (0.5, 3.0, 60, 900, 1.5) and args.pitch_track is True
        assert isinstance(args.track_lo, int) and mod.build_parser().parse_args(argv + ["--pitch-track"]).pitch_track is True
        with pytest.raises(ValueError, match="4001 states"):
            common.track_arguments(mod.build_parser().parse_args(argv + ["--track-lo", "95", "--track-hi", "4095"]))
        with pytest.raises(ValueError, match="--track-jump must be"):
            common.track_arguments(mod.build_parser().parse_args(argv + ["--track-jump", "-1"]))
