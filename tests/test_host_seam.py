"""CPU tests of the seam crossfade: the NumPy restatement tools/seam_ref.py (equal tail and head, a constant step spread over the fade,
Xe = min(X, stored), rows that are filling, off or do not fit, the gate's both-zero gains, shift = span + 1), seam_geometry's values
and errors, the validation of crossfade / crossfade_ms on a converter without a device, the C ABI's refusals, and the sessions file
("crossfade_ms" per session, --crossfade as the default; a file without the key loads to the settings it had)."""
import json
import os
import sys

import numpy as np
import pytest

from module import _native as nat
from module import multistream as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "alive-vc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import seam_ref as SR                                                # noqa: E402
import multistream_inference as MSI                                  # noqa: E402


# ------------------------------------------------------------------------------------------------ the restatement
def _row(ld=64, lo=10, sh=12, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((1, ld)).astype(np.float32), lo, sh


def test_identical_tail_and_head_leave_the_head_equal():
    y, lo, sh = _row()
    for x in (1, 5, 12):
        tail = np.zeros((1, 12), np.float32)
        tail[0, :x] = y[0, lo:lo + x]
        got, new_tail, stored, stats = SR.seam_rows(y, [lo], [sh], [x], [1], tail, [x])
        assert np.array_equal(got.view(np.int32), y.view(np.int32))      # t + (c - t) * w with c == t is t, whatever w
        assert np.array_equal(new_tail[0, :x], y[0, lo + sh:lo + sh + x]) and stored.tolist() == [x]
        assert stats[0, 0] == 0.0 and stats[0, 1] == SR.ordered_sum(y[0, lo:lo + x].astype(np.float64) ** 2) > 0
        assert SR.seam_db(stats)[0] == -np.inf


def test_a_constant_step_is_spread_evenly_over_the_fade():
    """the previous decode's continuation is a ramp r, this decode is r + d: a hard cut jumps by |d| (on top of the ramp's own
    increment) at the seam; the fade turns it into Xe + 1 increments of d / (Xe + 1) each"""
    ld, lo, sh, x, d, slope = 64, 8, 16, 15, 0.5, 2.0 ** -6
    t_axis = np.arange(-lo, ld - lo, dtype=np.float32)                   # time, 0 at the seam
    prev = (t_axis * np.float32(slope)).astype(np.float32)              # what the previous tick predicted for this tick's row
    cur = (prev + np.float32(d)).astype(np.float32)[None]
    tail = prev[None, lo:lo + x].copy()
    got, _, stored, stats = SR.seam_rows(cur, [lo], [sh], [x], [1], tail, [x])
    # the emitted join: the previous chunk ended on prev[lo - 1]; this one is got[lo:]
    join = np.concatenate([prev[lo - 1:lo], got[0, lo:lo + x + 1]]).astype(np.float64)
    inc = np.diff(join) - slope                                          # the increments beyond the ramp's own
    assert np.allclose(inc, d / (x + 1), rtol=0, atol=1e-6) and len(inc) == x + 1
    hard = np.diff(np.concatenate([prev[lo - 1:lo], cur[0, lo:lo + 2]]).astype(np.float64)) - slope
    assert abs(hard[0] - d) < 1e-6 and abs(hard[1]) < 1e-6               # the hard cut: the whole step at once
    assert np.array_equal(got[0, lo + x:], cur[0, lo + x:]) and np.array_equal(got[0, :lo], cur[0, :lo])
    assert stored.tolist() == [x] and abs(stats[0, 0] - x * d * d) < 1e-9
    w = SR.weights(x)
    assert w.dtype == np.float32 and 0 < w[0] and w[-1] < 1 and np.all(np.diff(w) > 0)
    assert np.array_equal(w, np.arange(1, x + 1, dtype=np.float32) / np.float32(x + 1))


def test_the_fade_covers_only_what_the_tail_holds():
    y, lo, sh = _row(seed=1)
    tail = np.full((1, 12), 7.0, np.float32)
    for x, stored, xe in ((8, 0, 0), (8, 3, 3), (8, 8, 8), (8, 11, 8), (12, 8, 8), (8, -2, 0)):
        got, new_tail, st, stats = SR.seam_rows(y, [lo], [sh], [x], [1], tail, [stored])
        want = y.copy()
        c = y[0, lo:lo + xe]
        want[0, lo:lo + xe] = np.float32(7.0) + (c - np.float32(7.0)) * SR.weights(xe)
        assert np.array_equal(got, want), (x, stored)
        assert st.tolist() == [x] and np.array_equal(new_tail[0, :x], y[0, lo + sh:lo + sh + x])
        assert np.array_equal(new_tail[0, x:], tail[0, x:])
        assert (stats[0, 1] > 0) == (xe > 0) and np.isnan(SR.seam_db(stats)[0]) == (xe == 0)


def test_rows_that_are_filling_off_or_do_not_fit():
    rng = np.random.default_rng(2)
    ld, ld_tail = 40, 10
    y = rng.standard_normal((9, ld)).astype(np.float32)
    tail = rng.standard_normal((9, ld_tail)).astype(np.float32)
    #        filling  off   lo<0  X<0  X>ld_tail  X>shift  past the row   fits exactly   fits
    lo = [5,      5,    -1,   5,   5,         5,       20,            20,            0]
    sh = [10,     10,   10,   10,  12,        4,       10,            10,            10]
    x = [6,       0,    6,    -3,  11,        5,       11,            10,            10]
    emit = [0, 1, 1, 1, 1, 1, 1, 1, 1]
    stored = np.full(9, 4, np.int32)
    got, new_tail, st, stats = SR.seam_rows(y, lo, sh, x, emit, tail, stored)
    assert np.array_equal(got[:7], y[:7]) and np.array_equal(new_tail[:7], tail[:7])
    assert st.tolist() == [4, 0, 0, 0, 0, 0, 0, 10, 10] and np.all(stats[:7] == 0)
    for r in (7, 8):
        assert not np.array_equal(got[r], y[r]) and np.array_equal(new_tail[r], y[r, lo[r] + sh[r]:lo[r] + sh[r] + 10])
        assert np.array_equal(got[r, lo[r] + 4:], y[r, lo[r] + 4:]) and stats[r, 1] > 0
    assert [SR.fits(a, b, c, ld, ld_tail) for a, b, c in zip(lo, sh, x)] == [True, True, False, False, False, False, False, True, True]


def test_a_tick_the_gate_skipped_leaves_nothing_to_fade_from():
    y, lo, sh = _row(seed=3)
    y = np.repeat(y, 4, axis=0)
    tail = np.ones((4, 12), np.float32)
    g0, g1 = [0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, 1.0]
    got, new_tail, st, stats = SR.seam_rows(y, [lo] * 4, [sh] * 4, [6] * 4, [1] * 4, tail, [6] * 4, g0, g1)
    assert st.tolist() == [0, 6, 6, 6]                                   # only closed at BOTH ends: that tick's search was skipped
    assert all(np.array_equal(got[r], got[3]) and np.array_equal(new_tail[r], new_tail[3]) for r in range(3))
    assert SR.seam_rows(y, [lo] * 4, [sh] * 4, [6] * 4, [1] * 4, tail, [6] * 4)[2].tolist() == [6] * 4
    # through stream(): speech, a closing tick, two skipped ticks, the reopening tick, speech -- the reopening chunk is not faded
    waves = [y[:1] + np.float32(t) for t in range(6)]
    gains = [None, ([1.0], [0.0]), ([0.0], [0.0]), ([0.0], [0.0]), ([0.0], [1.0]), ([1.0], [1.0])]
    faded, spans, stats, _, stored = SR.stream(waves, [lo], [12], [sh], [6], gains=gains)
    changed = [not np.array_equal(f, w) for f, w in zip(faded, waves)]
    assert changed == [False, True, True, False, False, True] and stored.tolist() == [6]
    assert all(s[0].shape == (12,) for s in spans) and np.array_equal(spans[4][0], waves[4][0, lo:lo + 12])


def test_the_tail_is_taken_one_chunk_on_not_one_span_on():
    """44.1 kHz under 160-sample ticks: chunk 441, span 440.  Successive waves are the same signal moved by 441 samples, so a tail
    taken at span_lo + 441 equals the next head exactly and the fade changes nothing; taken at span_lo + 440 it would not"""
    lo, span, shift, x, ld = 50, 440, 441, 220, 1400
    sig = np.random.default_rng(4).standard_normal(ld + 5 * shift).astype(np.float32)
    waves = [sig[t * shift:t * shift + ld][None] for t in range(5)]
    faded, spans, stats, tail, stored = SR.stream(waves, [lo], [span], [shift], [x])
    assert all(np.array_equal(f, w) for f, w in zip(faded, waves)) and stored.tolist() == [x]
    assert [float(s[0, 0]) for s in stats] == [0.0] * 5 and all(s[0, 1] > 0 for s in stats[1:]) and stats[0][0, 1] == 0
    assert all(s[0].shape == (span,) for s in spans)
    wrong = SR.stream(waves, [lo], [span], [span], [x])
    assert not any(np.array_equal(f, w) for f, w in zip(wrong[0][1:], waves[1:])) and all(s[0, 0] > 0 for s in wrong[2][1:])
    # a per-tick xlen: longer, then shorter; the fade is min(X, stored) long
    per = [[100], [100], [300], [300], [50]]
    _, _, st2, _, stored = SR.stream([w + np.float32(0.25 * t) for t, w in enumerate(waves)], [lo], [span], [shift], per, ld_tail=440)
    d2 = [s[0, 0] for s in st2]
    assert np.allclose(d2, [0, 100 / 16, 100 / 16, 300 / 16, 50 / 16], rtol=1e-6) and stored.tolist() == [50]


# ------------------------------------------------------------------------------------------------ the geometry
def test_seam_geometry_values():
    # (chunk_r, buffersize, rate): span_lo = bs * c // 2 - c // 2, shift = c, X = round(ms * rate / 1000)
    assert MS.seam_geometry(160, 16, 16000, 5, 2560) == (1200, 160, 80)
    assert MS.seam_geometry(160, 16, 16000, 10, 2560) == (1200, 160, 160)
    assert MS.seam_geometry(441, 16, 44100, 5, 7056) == (3308, 441, 220)      # span [3308, 3748): 440 samples, shift 441
    assert MS.seam_geometry(441, 16, 44100, 9.97, 7056) == (3308, 441, 440)
    assert MS.seam_geometry(480, 16, 48000, 5, 7680) == (3600, 480, 240)
    assert MS.seam_geometry(480, 16, 48000, 10, 7680) == (3600, 480, 480)
    assert MS.seam_geometry(480, 16, 48000, None, 7680) == (3600, 480, 0)
    assert MS.seam_geometry(160, 16, 16000, np.float32(2.5), 2560) == (1200, 160, 40)
    for c, bs in ((160, 16), (441, 16), (480, 16), (960, 8), (441, 7)):
        assert MS.seam_geometry(c, bs, 16000, None, 10 ** 6)[0] == bs * c // 2 - c // 2


def test_seam_geometry_errors():
    for bad in ("5", True, False, [5], float("nan"), float("inf"), 0, 0.0, -1, -0.5):
        with pytest.raises(ValueError, match=r"crossfade_ms=.* must be a finite number of milliseconds > 0, or None"):
            MS.seam_geometry(160, 16, 16000, bad, 2560)
    with pytest.raises(ValueError, match=r"crossfade_ms=10.1 is 162 samples at 16000 Hz.*takes 1 to 160 \(the largest crossfade_ms "
                                         r"that fits is 10\)"):
        MS.seam_geometry(160, 16, 16000, 10.1, 2560)
    with pytest.raises(ValueError, match=r"crossfade_ms=10 is 441 samples at 44100 Hz.*takes 1 to 440 \(the largest crossfade_ms that "
                                         r"fits is 9.97732\)"):
        MS.seam_geometry(441, 16, 44100, 10, 7056)                       # one more than the span of 440
    with pytest.raises(ValueError, match=r"crossfade_ms=0.01 is 0 samples"):
        MS.seam_geometry(160, 16, 16000, 0.01, 2560)
    # the wave ends before span_lo + shift + X: 1200 + 160 + 80 = 1440
    assert MS.seam_geometry(160, 16, 16000, 5, 1440) == (1200, 160, 80)
    with pytest.raises(ValueError, match=r"in a wave of 1439 takes 1 to 79 \(the largest crossfade_ms that fits is 4.9375\)"):
        MS.seam_geometry(160, 16, 16000, 5, 1439)
    with pytest.raises(ValueError, match=r"takes 1 to 0 \(the largest crossfade_ms that fits is 0\)"):
        MS.seam_geometry(160, 16, 16000, 5, 1300)


# ------------------------------------------------------------------------------------------------ the settings
def _host_converter(crossfade, rates=None):
    """the part of a converter the crossfade's validation reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.crossfade, c.chunk, c.buffersize, c.input_sr = crossfade, 160, 16, 16000
    c._rt, c.rate = None, [16000, 16000, 44100]
    c._row_len = {16000: 2560}
    if rates:
        c._rt, c._chunks, c._row_len = object(), {16000: 160, 44100: 441, 48000: 480}, {16000: 2560, 44100: 7056, 48000: 7680}
    return c


def test_session_crossfade_is_checked_against_the_converter():
    assert "crossfade_ms" in MS._PARAMS
    on, off, multi = _host_converter(True), _host_converter(False), _host_converter(True, rates=True)
    assert on._session_seam(0, dict(crossfade_ms=5)) == 80 and on._session_seam(0, dict(crossfade_ms=10.0)) == 160
    assert on._session_seam(0, dict(crossfade_ms=None)) == 0 == on._session_seam(0, {}) == off._session_seam(1, {})
    assert multi._session_seam(2, dict(crossfade_ms=5)) == 220           # the slot's own rate, 44.1 kHz
    assert multi._session_seam(0, dict(crossfade_ms=5), 48000) == 240    # open(): the rate the slot is about to take
    with pytest.raises(ValueError, match=r"slot 2: crossfade_ms=5 needs a converter built with MultiStreamConverter\(..., "
                                         r"crossfade=True\)"):
        off._session_seam(2, dict(crossfade_ms=5))
    for bad in ("5", True, float("nan"), float("inf"), 0, -3):
        for c in (on, off):
            with pytest.raises(ValueError, match="slot 1: crossfade_ms=.* must be a finite number of milliseconds > 0"):
                c._session_seam(1, dict(crossfade_ms=bad))
    with pytest.raises(ValueError, match=r"slot 1: crossfade_ms=11 is 176 samples at 16000 Hz.*largest crossfade_ms that fits is 10"):
        on._session_seam(1, dict(crossfade_ms=11))
    with pytest.raises(ValueError, match=r"slot 2: crossfade_ms=10 is 441 samples at 44100 Hz"):
        multi._session_seam(2, dict(crossfade_ms=10))
    with pytest.raises(ValueError, match="crossfade must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, crossfade=1)
    with pytest.raises(ValueError, match=r"crossfade=True needs input_sr == output_sr \(got 16000 and 48000\).*not a whole number"):
        MS.MultiStreamConverter(None, None, None, None, 1, crossfade=True, output_sr=48000)
    with pytest.raises(ValueError, match=r"seam_db needs a converter built with MultiStreamConverter\(..., crossfade=True\)"):
        off.seam_db()
    assert MS.stats_db([(0.0, 0.0), (1.0, 100.0), (0.0, 4.0)])[1:] == [-20.0, -np.inf] and np.isnan(MS.stats_db([(0.0, 0.0)])[0])


def test_realtime_converter_checks_its_crossfade_before_anything_is_built():
    from module.realtime import RealtimeConverter
    for bad in ("5", True, 0, float("nan")):
        with pytest.raises(ValueError, match="crossfade_ms=.* must be a finite number of milliseconds > 0"):
            RealtimeConverter(None, None, None, None, crossfade_ms=bad)
    with pytest.raises(ValueError, match=r"crossfade_ms needs input_sr == output_sr \(got 16000 and 48000\)"):
        RealtimeConverter(None, None, None, None, crossfade_ms=5, output_sr=48000)
    rt = RealtimeConverter.__new__(RealtimeConverter)
    rt.crossfade = False
    with pytest.raises(ValueError, match=r"seam_db needs a converter built with RealtimeConverter\(..., crossfade_ms=MS\)"):
        rt.seam_db()


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_seam_abi_refuses_bad_arguments():
    L = nat.lib()
    #     y   N  ld  lo  shift xlen emit g0    g1    tail ld_tail stored stats stream
    ok = [16, 2, 64, 16, 16,   16,  16,  None, None, 16,  8,      16,    None, None]
    for i in (0, 3, 4, 5, 6, 9, 11):
        a = list(ok)
        a[i] = None
        assert L.alive_seam_rows(*a) == -1 and b"null" in L.alive_last_error(), i
    for i in (7, 8):                                                     # exactly one of g0 / g1
        a = list(ok)
        a[i] = 16
        assert L.alive_seam_rows(*a) == -1 and b"go together" in L.alive_last_error(), i
    for i, bad in ((1, 0), (1, -1), (2, 0), (2, -5), (10, 0), (10, -1)):
        a = list(ok)
        a[i] = bad
        assert L.alive_seam_rows(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)


# ------------------------------------------------------------------------------------------------ the sessions file
@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "spk.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, entries, name="f.json"):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_sessions_file_takes_a_crossfade_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, crossfade_ms=10), dict(sess, crossfade_ms=2.5)]))
    assert "crossfade_ms" not in a and (b["crossfade_ms"], c["crossfade_ms"]) == (10.0, 2.5)
    assert isinstance(b["crossfade_ms"], float)
    # --crossfade is the default; a session's null switches it off, its own value wins
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, crossfade_ms=None), dict(sess, crossfade_ms=3)]), crossfade_ms=8)
    assert a["crossfade_ms"] == 8.0 and "crossfade_ms" not in b and c["crossfade_ms"] == 3.0
    for bad in ("10", True, [1], {"ms": 1}, 0, -5):
        with pytest.raises(ValueError, match=r"session 1: crossfade_ms="):
            MSI.load_sessions(write(files, [sess, dict(sess, crossfade_ms=bad)]))
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['crossfade'\]"):
        MSI.load_sessions(write(files, [dict(sess, crossfade=10)]))
    with pytest.raises(ValueError, match=r"--crossfade: crossfade_ms="):
        MSI.load_sessions(write(files, [sess]), crossfade_ms=float("nan"))
    with pytest.raises(ValueError, match=r"--crossfade: crossfade_ms="):
        MSI.load_sessions(write(files, [sess]), crossfade_ms=0)


def test_a_sessions_file_without_the_key_loads_to_the_settings_it_had(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    plain = MSI.load_sessions(write(files, [dict(sess, pitch=3, sr=48000)]), k=6)[0]
    assert plain == dict(input=str(files / "a.wav"), target=None, lib=str(files / "voice_library.pt"), output=None, pitch=3.0,
                         f0_rate=1.0, alpha=0.0, gain=0.0, input_gain=0.0, start=0, sr=48000, world_pitch=False, blend=None, k=6,
                         auto_pitch=False, register_hz=None)
    args = MSI.build_parser().parse_args(["s.json"])
    assert args.crossfade is None
    assert MSI.build_parser().parse_args(["s.json", "--crossfade", "7.5"]).crossfade == 7.5


def test_realtime_cli_takes_the_crossfade():
    import realtime_inference as RI
    assert RI.build_parser().parse_args([]).crossfade is None
    assert RI.build_parser().parse_args(["-xf", "5"]).crossfade == 5.0
    assert RI.build_parser().parse_args(["--crossfade", "2.5"]).crossfade == 2.5
