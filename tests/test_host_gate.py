"""CPU tests of the input gate: the NumPy restatement tools/gate_ref.py (hold sequences, rows that are off or filling, the ramp, the
ordered mean square), the threshold and hold derived from the arguments, the session settings' validation on a converter without a
device, the C ABI's refusals, and the sessions file ("gate_db" / "gate_hold" per session, -thr / --gate-hold as defaults; a file
without the keys loads to the settings it had)."""
import json
import math
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
import gate_ref as GR                                                # noqa: E402
import multistream_inference as MSI                                  # noqa: E402


# ------------------------------------------------------------------------------------------------ the restatement
def _run(loud, hold, gate_on=1, emit=None, state=(0, 0)):
    """one row through a loud / quiet script -> [(g0, g1, open, left, seg_len_eff, follow)] per tick"""
    st, out = np.array([state], dtype=np.int32), []
    for t, l in enumerate(loud):
        e = 1 if emit is None else emit[t]
        r = GR.gate_rows(st, [1.0 if l else 0.0], [gate_on], [0.5], [hold], [e], [7])
        st = r["state"]
        out.append((float(r["g0"][0]), float(r["g1"][0]), bool(r["open"][0]), int(st[0, 0]), int(r["seg_len_eff"][0]),
                    bool(r["follow"][0])))
    return out


def test_a_gate_stays_open_for_exactly_hold_ticks_after_the_last_loud_one():
    for hold in (0, 1, 3):
        loud = [0, 1, 1] + [0] * (hold + 3) + [1, 0]
        got = _run(loud, hold)
        want_open = [False, True, True] + [True] * hold + [False] * 3 + [True] + [hold > 0]
        assert [g[2] for g in got] == want_open, hold
        # g0 is the previous tick's open, g1 this tick's; a row closed at both ends is skipped, and only then
        prev = False
        for (g0, g1, is_open, left, seg, follow), l in zip(got, loud):
            assert (g0, g1) == (float(prev), float(is_open)) and follow == is_open
            assert seg == (0 if not prev and not is_open else 7)
            assert left == (hold if l else left) and 0 <= left <= hold
            prev = is_open


def test_hold_zero_closes_on_the_first_quiet_tick_with_a_fade_out():
    got = _run([1, 0, 0], 0)
    assert [(g[0], g[1], g[4]) for g in got] == [(0.0, 1.0, 7), (1.0, 0.0, 7), (0.0, 0.0, 0)]


def test_rows_that_are_off_or_filling_pass_everything_and_keep_their_state():
    for gate_on, emit in ((0, 1), (1, 0), (0, 0)):
        r = GR.gate_rows([[2, 1]], [0.0], [gate_on], [0.5], [5], [emit], [3, 4], S=2, world_on=[1])
        assert r["state"].tolist() == [[2, 1]] and r["g0"].tolist() == [1.0] and r["g1"].tolist() == [1.0]
        assert r["seg_len_eff"].tolist() == [3, 4] and r["follow"].tolist() == [bool(emit)] and r["world_eff"].tolist() == [1]
    # a filling row in the middle of a script does not count down its hold
    got = _run([1, 0, 0, 0, 0], 2, emit=[1, 0, 0, 1, 1])
    assert [g[3] for g in got] == [2, 2, 2, 1, 0] and [g[2] for g in got] == [True, True, True, True, True]


def test_world_mask_and_list_rows_follow_the_skip():
    st = [[0, 0], [0, 1], [1, 0], [0, 0]]
    r = GR.gate_rows(st, [0.0, 0.0, 0.0, 1.0], [1] * 4, [0.5] * 4, [2] * 4, [1] * 4, list(range(1, 9)), S=2, world_on=[1, 1, 1, 0])
    assert r["g0"].tolist() == [0, 1, 0, 0] and r["g1"].tolist() == [0, 0, 1, 1]
    assert r["seg_len_eff"].tolist() == [0, 0, 3, 4, 5, 6, 7, 8] and r["world_eff"].tolist() == [0, 1, 1, 0]
    assert r["state"].tolist() == [[0, 0], [0, 0], [0, 1], [2, 1]]
    assert GR.gate_rows(st, [0.0] * 4, [1] * 4, [0.5] * 4, [2] * 4, [1] * 4, [1] * 4)["world_eff"] is None


def test_the_threshold_edge_is_inclusive_and_the_ordered_sum_is_exact_on_a_constant():
    x = np.full((2, 2560), 0.5, dtype=np.float32)
    ms = GR.mean_square(x, 1200, 1520)
    assert ms.tolist() == [0.25, 0.25]
    assert GR.gate_rows([[0, 0]], ms[:1], [1], [0.25], [0], [1], [1])["open"].tolist() == [True]
    assert GR.gate_rows([[0, 0]], ms[:1], [1], [np.nextafter(0.25, 1.0)], [0], [1], [1])["open"].tolist() == [False]
    rng = np.random.default_rng(3)
    y = rng.standard_normal((3, 1000)).astype(np.float32)
    for lo, hi in ((0, 1000), (17, 18), (100, 613)):
        want = (y[:, lo:hi].astype(np.float64) ** 2).mean(axis=1)
        assert np.all(np.abs(GR.mean_square(y, lo, hi) - want) <= 1e-12 * want)


def test_the_ramp_is_float32_ends_on_g1_and_apply_leaves_the_rest_alone():
    for n in (1, 2, 441, 480):
        up, down = GR.ramp(0, 1, n), GR.ramp(1, 0, n)
        assert up.dtype == np.float32 and up[-1] == 1.0 and down[-1] == 0.0 and np.all(np.diff(up) > 0)
        t = np.arange(1, n + 1, dtype=np.float32) / np.float32(n)
        assert np.array_equal(down, np.float32(1.0) + np.float32(-1.0) * t)
    y = np.arange(1, 41, dtype=np.float32).reshape(4, 10)
    y[3, 2] = np.nan
    got = GR.apply_rows(y, [2, 8, 0, 1], [4, 4, 3, 3], [1, 0, 1, 0], [1, 1, 0, 0])
    assert np.array_equal(got[0], y[0])
    assert np.array_equal(got[1], np.concatenate([y[1, :8], y[1, 8:] * GR.ramp(0, 1, 4)[:2]]))         # clamped by the row's end
    assert np.array_equal(got[2], np.concatenate([y[2, :3] * GR.ramp(1, 0, 3), y[2, 3:]]))
    assert got[3].tolist() == [31.0, 0.0, 0.0, 0.0] + y[3, 4:].tolist() and not np.signbit(got[3, 1:4]).any()


# ------------------------------------------------------------------------------------------------ the settings
def test_threshold_and_hold_are_derived_in_float64_on_the_host():
    for db in (-40, -40.0, -23.5, 0, 3, np.float32(-60.0)):
        assert MS.gate_thr_ms(db) == 10.0 ** (float(db) / 10.0) == GR.thr_ms(db)
    assert MS.gate_thr_ms(-40) == 1e-4 and MS.gate_thr_ms(0) == 1.0
    tick = 160 / 16000
    for hold, want in ((0, 0), (0.0, 0), (0.001, 1), (0.01, 1), (0.011, 2), (0.2, 20), (0.205, 21), (1, 100)):
        assert MS.gate_hold_ticks(hold, tick) == want == GR.hold_ticks(hold, tick) == math.ceil(hold / tick), hold
    assert MS.gate_hold_ticks(0.2, 960 / 16000) == 4
    for bad in (None, "x", True, float("nan"), float("inf"), -float("inf"), [1]):
        with pytest.raises(ValueError, match="gate_db=.* must be a finite number of dBFS"):
            MS.gate_thr_ms(bad)
    for bad in (None, "x", False, float("nan"), float("inf"), -0.01, -1):
        with pytest.raises(ValueError, match="gate_hold=.* must be a finite number of seconds >= 0"):
            MS.gate_hold_ticks(bad, tick)
    assert MS.gate_window(1200, 1360, 2560, 160) == (1200, 1520) and MS.gate_window(1200, 1360, 1400, 160) == (1200, 1400)


def _host_converter(gate):
    """the part of a converter the gate's validation reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.gate, c.chunk, c.input_sr = gate, 160, 16000
    return c


def test_session_gate_settings_are_checked_against_the_converter():
    assert {"gate_db", "gate_hold"} <= set(MS._PARAMS)
    on, off = _host_converter(True), _host_converter(False)
    assert on._session_gate(0, dict(gate_db=-40, gate_hold=0.03)) == (1, 1e-4, 3)
    assert on._session_gate(0, dict(gate_db=-40)) == (1, 1e-4, 20)                      # the default hold, 0.2 s
    assert on._session_gate(0, dict(gate_db=None, gate_hold=0.5)) == (0, 0.0, 0)
    assert on._session_gate(0, {}) == (0, 0.0, 0) == off._session_gate(1, {})
    with pytest.raises(ValueError, match=r"slot 2: gate_db=-40 needs a converter built with MultiStreamConverter\(..., gate=True\)"):
        off._session_gate(2, dict(gate_db=-40))
    for bad in ("loud", True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="slot 1: gate_db="):
            on._session_gate(1, dict(gate_db=bad))
    for bad in (-0.1, None, "1", float("nan")):
        with pytest.raises(ValueError, match="slot 1: gate_hold="):
            on._session_gate(1, dict(gate_db=-40, gate_hold=bad))
        with pytest.raises(ValueError, match="slot 1: gate_hold="):
            off._session_gate(1, dict(gate_hold=bad))
    with pytest.raises(ValueError, match="gate must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, gate=1)
    with pytest.raises(ValueError, match="gate_lookahead=-1 must be >= 0 seconds"):
        MS.MultiStreamConverter(None, None, None, None, 1, gate=True, gate_lookahead=-1)


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_gate_abi_refuses_bad_arguments():
    L = nat.lib()
    ok = [16, 2, 64, 8, 40, 16, 16, 16, 16, None, 1, 16, 16, 16, 16, 16, 16, None, None, None]
    for i in (0, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16):
        a = list(ok)
        a[i] = None
        assert L.alive_gate_rows(*a) == -1 and b"null" in L.alive_last_error(), i
    for i in (9, 17):                                                    # world_on and world_eff go together
        a = list(ok)
        a[i] = 16
        assert L.alive_gate_rows(*a) == -1 and b"go together" in L.alive_last_error()
    for i, bad in ((1, 0), (2, 0), (10, 0)):
        a = list(ok)
        a[i] = bad
        assert L.alive_gate_rows(*a) == -1, (i, bad)
    for lo, hi in ((-1, 8), (8, 8), (9, 8), (0, 65)):
        a = list(ok)
        a[3], a[4] = lo, hi
        assert L.alive_gate_rows(*a) == -1 and b"outside [0, 64) or empty" in L.alive_last_error()
    ok = [16, 2, 64, 16, 16, 16, 16, None]
    for i in (0, 3, 4, 5, 6):
        a = list(ok)
        a[i] = None
        assert L.alive_gate_apply_rows(*a) == -1 and b"null" in L.alive_last_error()
    for i, bad in ((1, 0), (1, 65536), (2, 0), (2, 1 << 30)):
        a = list(ok)
        a[i] = bad
        assert L.alive_gate_apply_rows(*a) == -1 and b"bad args" in L.alive_last_error()


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


def test_sessions_file_takes_a_gate_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, gate_db=-40), dict(sess, gate_db=-35.5, gate_hold=0)]))
    assert "gate_db" not in a and "gate_hold" not in a
    assert (b["gate_db"], b["gate_hold"], c["gate_db"], c["gate_hold"]) == (-40.0, 0.2, -35.5, 0.0)
    # -thr / --gate-hold are the defaults; a session's null switches its gate off, its own values win
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, gate_db=None), dict(sess, gate_db=-20, gate_hold=1)]), gate_db=-50,
                                gate_hold=0.1)
    assert (a["gate_db"], a["gate_hold"]) == (-50.0, 0.1) and "gate_db" not in b and (c["gate_db"], c["gate_hold"]) == (-20.0, 1.0)
    for bad in ("-40", True, [1], {"db": 1}):
        with pytest.raises(ValueError, match=r"session 1: gate_db="):
            MSI.load_sessions(write(files, [sess, dict(sess, gate_db=bad)]))
    for bad in (-1, "0.2", None, True):
        with pytest.raises(ValueError, match=r"session 0: gate_hold="):
            MSI.load_sessions(write(files, [dict(sess, gate_db=-40, gate_hold=bad)]))
    with pytest.raises(ValueError, match=r"session 0: gate_hold="):              # mistyped even on a session without a gate
        MSI.load_sessions(write(files, [dict(sess, gate_hold=-2)]))
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['gate'\]"):
        MSI.load_sessions(write(files, [dict(sess, gate=-40)]))
    with pytest.raises(ValueError, match=r"-thr / --gate-hold: gate_hold="):
        MSI.load_sessions(write(files, [sess]), gate_hold=-1)
    with pytest.raises(ValueError, match=r"-thr / --gate-hold: gate_db="):
        MSI.load_sessions(write(files, [sess]), gate_db=float("nan"))


def test_a_sessions_file_without_the_keys_loads_to_the_settings_it_had(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    plain = MSI.load_sessions(write(files, [dict(sess, pitch=3, sr=48000)]), k=6)[0]
    assert plain == dict(input=str(files / "a.wav"), target=None, lib=str(files / "voice_library.pt"), output=None, pitch=3.0,
                         f0_rate=1.0, alpha=0.0, gain=0.0, input_gain=0.0, start=0, sr=48000, world_pitch=False, blend=None, k=6,
                         auto_pitch=False, register_hz=None)
    args = MSI.build_parser().parse_args(["s.json"])
    assert args.gate_db is None and args.gate_hold == 0.2
    args = MSI.build_parser().parse_args(["s.json", "-thr", "-42.5", "--gate-hold", "0.05"])
    assert (args.gate_db, args.gate_hold) == (-42.5, 0.05)
    assert MSI.build_parser().parse_args(["s.json", "--gate-db", "-30"]).gate_db == -30.0


def test_realtime_cli_takes_the_threshold():
    import realtime_inference as RI
    args = RI.build_parser().parse_args([])
    assert args.threshold is None and args.gate_hold == 0.2
    args = RI.build_parser().parse_args(["-thr", "-45", "--gate-hold", "0.1"])
    assert (args.threshold, args.gate_hold) == (-45.0, 0.1)
    assert RI.build_parser().parse_args(["--threshold", "-30"]).threshold == -30.0
