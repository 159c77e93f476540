"""CPU tests of loudness normalisation: the NumPy restatement tools/loudness_ref.py (the standard's 48-kHz coefficients, the 997-Hz
reference tone, the tiled filter against the end-to-end recurrence, the two gates, the streaming follower's properties), the host's
numbers in module/multistream.py against the restatement's bit for bit, check_loudness with every refusal, the validation on converters
without a device, the sessions and jobs files, the CLIs' flags, and the C ABI (symbols, prototypes, refusals)."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest

from module import _native as nat
from module import multistream as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "alive-vc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import loudness_ref as R                                             # noqa: E402
import batch_inference as BI                                         # noqa: E402
import multistream_inference as MSI                                  # noqa: E402

Z_ABS = R.z_of(-70.0)


def tone(fs, seconds, amplitude=1.0, hz=997.0):
    return (amplitude * np.sin(2.0 * np.pi * hz * np.arange(int(round(seconds * fs))) / fs)).astype(np.float32)


def integrated(y, fs, tiled=True):
    """the integrated loudness of y in LUFS by the restatement"""
    H, c = R.hop(fs), R.coefficients(fs)
    q = R.tile_q(y, H, c) if tiled else R.plain_q(y, H, c)
    return float(R.lufs(R.gate(R.blocks(q, H), Z_ABS)[0]))


# ------------------------------------------------------------------------------------------------ the measurement
def test_the_48_khz_coefficients_are_the_standards_table():
    table = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    assert np.max(np.abs(R.coefficients(48000) - np.array(table))) <= 1e-12
    assert [R.hop(fs) for fs in (8000, 16000, 44100, 48000, 22050)] == [800, 1600, 4410, 4800, 2205]


def test_the_reference_tone_reads_what_the_standard_says():
    assert abs(integrated(tone(48000, 1.0), 48000) - (-3.01)) <= 0.01
    # at 16 kHz the re-derived filter has its own gain at 997 Hz: -2.970, not a tolerance on -3.01
    assert abs(integrated(tone(16000, 1.0), 16000) - (-2.970)) <= 0.005
    for fs in (48000, 16000):
        for short in (0, 4 * R.hop(fs) - 1):                          # fewer than four sub-blocks: nothing to measure
            H, c = R.hop(fs), R.coefficients(fs)
            assert R.gate(R.blocks(R.tile_q(tone(fs, 1.0)[:short], H, c), H), Z_ABS) == (0.0, 0, 0)
    assert R.lufs(0.0) == -np.inf and abs(float(R.lufs(R.z_of(-23.0))) + 23.0) < 1e-12


@pytest.mark.parametrize("fs", [8000, 16000, 44100, 48000])
def test_the_tiled_filter_is_the_end_to_end_recurrence_up_to_rounding(fs):
    rng = np.random.default_rng(fs)
    y = (0.1 * rng.standard_normal(2 * fs + 37)).astype(np.float32)
    y[fs // 2:] += np.float32(0.3)                                    # a DC step: the high-pass state has to be carried exactly
    H, c = R.hop(fs), R.coefficients(fs)
    a, b = R.tile_q(y, H, c), R.plain_q(y, H, c)
    assert a.shape == b.shape == ((2 * fs + 37) // H,)
    assert np.max(np.abs(a - b) / b) <= 1e-11
    # the carry matrix really is the zero-input response: column k from unit state k
    AP = R.carry_matrix(c, H)
    for k in range(4):
        assert np.array_equal(AP[:, k], R.run(np.zeros((1, H)), c, np.eye(4)[k:k + 1])[0][0])
    # a non-finite sample counts as 0.0
    z = y.copy()
    z[[5, 900, fs]] = [np.nan, np.inf, -np.inf]
    w = y.copy()
    w[[5, 900, fs]] = 0.0
    assert np.array_equal(R.tile_q(z, H, c), R.tile_q(w, H, c))


def test_the_relative_gate_drops_the_quiet_stretches():
    fs = 16000
    amp = lambda level: 10.0 ** ((level + 2.970) / 20.0)              # noqa: E731  (full scale reads -2.970 at 16 kHz)
    y = np.concatenate([tone(fs, 2.0, amp(-36)), tone(fs, 4.0, amp(-23)), tone(fs, 2.0, amp(-36))])
    H, c = R.hop(fs), R.coefficients(fs)
    z = R.blocks(R.tile_q(y, H, c), H)
    zI, c1, c2 = R.gate(z, Z_ABS)
    gated, plain = float(R.lufs(zI)), float(R.lufs(R.ungated(z)))
    assert -23.5 <= gated <= -23.0 and gated >= plain + 2.0
    assert c1 == len(z) == 77 and 0 < c2 < c1
    # silence: under the absolute gate, nothing is counted, and the gain stays at 1
    assert R.gate(R.blocks(R.tile_q(np.zeros(fs, np.float32), H, c), H), Z_ABS) == (0.0, 0, 0)
    assert R.gain(0.0, 0, R.z_of(-23), 4.0) == 1.0 and R.gain(1e-3, 5, math.nan, 4.0) == 1.0
    assert R.gain(R.z_of(-60), 5, R.z_of(-23), 10 ** 0.6) == 10 ** 0.6 and R.gain(R.z_of(-3), 5, R.z_of(-23), 10 ** 0.6) == 1 / 10 ** 0.6


# ------------------------------------------------------------------------------------------------ the streaming follower
def _run_stream(y, fs, n, target, state=None, **kw):
    """y in spans of n through loudness_rows -> (out, the gain after every tick, the state after every tick)"""
    H, c, par = R.hop(fs), R.coefficients(fs), R.params(fs, n, target, **kw)
    st = R.state0(1) if state is None else state
    out, gains, states = [], [], []
    for t in range(len(y) // n):
        w, st = R.loudness_rows(y[None, t * n:(t + 1) * n], [0], [n], [1], [1], [H], [c], par[None], st)
        out.append(w[0])
        gains.append(st[0, R.G_SLOT])
        states.append(st[0].copy())
    return np.concatenate(out), np.array(gains), states


def test_the_follower_reaches_its_target_within_its_slew_and_range():
    fs, n = 16000, 160
    y = tone(fs, 4.0, 10.0 ** ((-30 + 2.970) / 20.0))                  # reads -30 LUFS at 16 kHz
    out, g, states = _run_stream(y, fs, n, -20.0)
    qs = R.params(fs, n, -20.0)[5]
    assert abs(20 * np.log10(g[3 * fs // n - 1]) - 10.0) <= 0.1       # within 0.1 dB of the target by 3 s
    steps = np.concatenate([[g[0]], g[1:] / g[:-1]])
    assert np.all(steps <= qs) and np.all(steps >= 1.0 / qs)          # no tick moves the gain by more than its qs
    assert abs(R.running_lufs(states[-1]) + 30.0) < 0.01
    assert abs(integrated(out[3 * fs:], fs) + 20.0) < 0.1             # what is emitted reads the target
    # a target out of reach: the gain stops at gmax
    out, g, _ = _run_stream(y, fs, n, -5.0, max_db=12.0, slew=60.0)
    assert np.all(g <= 10 ** 0.6) and g[-1] == 10 ** 0.6
    out, g, _ = _run_stream(tone(fs, 3.0, 0.9), fs, n, -40.0, max_db=6.0, slew=60.0)
    assert np.all(g >= 1 / 10 ** 0.3) and g[-1] == 1 / 10 ** 0.3


def test_silence_leaves_the_running_loudness_and_the_gains_target_alone():
    fs, n = 16000, 160
    loud = tone(fs, 2.0, 10.0 ** ((-30 + 2.970) / 20.0))
    # S and W decay by d with every sub-block whatever it holds, so "unchanged" is their ratio, the running loudness, and with it the
    # gain's target.  The 400 ms after the tone still end blocks that hold part of it: those count, so the state is taken after them
    _, _, states = _run_stream(np.concatenate([loud, np.zeros(4 * R.hop(fs), np.float32)]), fs, n, -20.0)
    par = R.params(fs, n, -20.0)
    want = R.target_gain(states[-1], par)
    _, _, after = _run_stream(np.zeros(fs, np.float32), fs, n, -20.0, state=states[-1][None].copy())
    S0, W0 = states[-1][10], states[-1][11]
    S1, W1 = after[-1][10], after[-1][11]
    assert 0 < W1 < W0 and abs(S1 / W1 - S0 / W0) <= 1e-12 * (S0 / W0)      # both decay together: the mean stands
    # W stays above the prior here, so the target of the gain is the same up to the rounding of S / W
    assert W1 >= par[3] and abs(R.target_gain(after[-1], par) - want) <= 1e-12 * want
    # and a stream that has heard nothing but silence stays at gain 1, bit for bit
    out, g, st = _run_stream(np.zeros(fs, np.float32), fs, n, -20.0)
    assert np.all(g == 1.0) and st[-1][10] == 0.0 and st[-1][11] == 0.0 and not out.any()


def test_a_quiet_talker_is_a_pause_until_the_prior_has_decayed():
    fs, n = 16000, 160
    amp = lambda level: 10.0 ** ((level + 2.970) / 20.0)              # noqa: E731
    _, _, a = _run_stream(tone(fs, 3.0, amp(-25)), fs, n, -20.0)
    _, _, b = _run_stream(tone(fs, 12.0, amp(-45)), fs, n, -20.0, state=a[-1][None].copy())
    par = R.params(fs, n, -20.0)
    early, late = b[fs // n], b[-1]                                   # 1 s in: gated out, W still trusted; 12 s in: believed
    # (the three blocks that straddle the drop hold 3/4, 1/2 and 1/4 of the loud level and pass the relative gate: among W > 18
    # counted blocks they pull the mean down by less than 1.5 / 18 = 8 %, 0.4 dB; nothing of the quiet talker itself is counted)
    assert early[11] >= par[3] and -25.5 < R.running_lufs(early) < -25.0
    # afterwards one quiet block is let in whenever W has fallen under P, so W hovers at the prior while the loud blocks decay out of
    # S: four half-lives on a sixteenth of them is left among ten blocks, and the running loudness has fallen by most of 10 dB
    assert par[3] * par[2] <= late[11] <= par[3] + 1.0 and -36.0 < R.running_lufs(late) < -31.0


def test_the_state_does_not_depend_on_how_the_stream_is_cut():
    fs = 16000
    rng = np.random.default_rng(7)
    y = (0.05 * rng.standard_normal(fs + 1600)).astype(np.float32)
    y[4000:9000] *= np.float32(0.001)
    ends = []
    for n in (160, 441, 1600, 2200, fs + 1600):                       # 2200 and the whole: more than one sub-block per span
        m = (len(y) // n) * n
        _, _, st = _run_stream(y[:m], fs, n, -23.0)
        # the rest in one more span, so that every cut has seen the same samples
        if m < len(y):
            H, c = R.hop(fs), R.coefficients(fs)
            _, last = R.loudness_rows(y[None, m:], [0], [len(y) - m], [1], [1], [H], [c], R.params(fs, len(y) - m, -23.0)[None],
                                      st[-1][None].copy())
            ends.append(last[0])
        else:
            ends.append(st[-1])
    for e in ends[1:]:
        assert np.array_equal(e[:12].view(np.int64), ends[0][:12].view(np.int64))      # the filter, the open sub-block, S and W


def test_rows_that_are_off_absent_or_do_not_fit():
    fs, n = 16000, 160
    H, c, par = R.hop(fs), R.coefficients(fs), R.params(fs, n, -20.0)
    y = np.stack([tone(fs, 0.02, 0.3)[:320]] * 5)
    st = R.state0(5)
    st[:, 10:13] = [[3e-3, 5.0, 1.5]] * 5
    #           on    absent  off   span past the row   hop 0
    emit, on = [1, 0, 1, 1, 1], [1, 1, 0, 1, 1]
    out, after = R.loudness_rows(y, [0, 0, 0, 200, 0], [n] * 5, emit, on, [H, H, H, H, 0], [c] * 5, np.stack([par] * 5), st)
    assert not np.array_equal(out[0], y[0]) and np.array_equal(out[0, n:], y[0, n:])
    assert np.array_equal(out[1:], y[1:])
    assert np.array_equal(after[1], st[1])
    for r in (2, 3, 4):
        assert np.array_equal(after[r], R.state0(1)[0])


# ------------------------------------------------------------------------------------------------ the host's numbers
@pytest.mark.parametrize("fs", [8000, 16000, 22050, 44100, 48000])
def test_the_products_host_numbers_are_the_restatements(fs):
    coef, ap = MS.loudness_filter(fs)
    c = R.coefficients(fs)
    assert np.array_equal(np.array(coef), c) and MS.loudness_hop(fs) == R.hop(fs)
    assert np.array_equal(np.array(ap).reshape(4, 4), R.carry_matrix(c, R.hop(fs)))
    assert MS.loudness_z(-23.0) == R.z_of(-23.0) and MS.loudness_lufs(R.z_of(-23.0)) == float(R.lufs(R.z_of(-23.0)))
    assert MS.loudness_lufs(0.0) == -math.inf
    d, P, z_abs, gmax, slew = MS.check_loudness_stream()
    want = R.params(fs, 160, -20.0)
    got = (z_abs, MS.check_loudness(-20.0)[0], d, P, gmax, MS.loudness_slew(slew, 160, fs))
    assert np.array_equal(np.array(got), want)
    assert (MS.LOUDNESS_STATE, MS.LOUDNESS_PARAMS) == (R.STATE, R.PARAMS)
    hdr = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    assert int(re.search(r"#define ALIVE_LOUDNESS_STATE (\d+)", hdr).group(1)) == MS.LOUDNESS_STATE
    assert int(re.search(r"#define ALIVE_LOUDNESS_PARAMS (\d+)", hdr).group(1)) == MS.LOUDNESS_PARAMS


def test_check_loudness_is_the_one_rule_set():
    assert MS.check_loudness(None) is None and MS.check_loudness(None, 3) is None
    assert MS.check_loudness(-23) == (R.z_of(-23.0), 10 ** 0.6) and MS.check_loudness(0, 0) == (R.z_of(0.0), 1.0)
    assert MS.check_loudness(np.float32(-16), np.int64(6)) == (R.z_of(-16.0), 10 ** 0.3)
    for bad in ("-23", True, [1], float("nan"), float("-inf"), 0.5, -70, -71):
        with pytest.raises(ValueError, match=r"lufs=.* must be a finite number of LUFS in \(-70, 0\], or None"):
            MS.check_loudness(bad)
    for bad in ("6", True, None, float("nan"), float("inf"), -1):
        for target in (None, -23):
            with pytest.raises(ValueError, match=r"loudness max gain .* must be a finite number of dB >= 0"):
                MS.check_loudness(target, bad)
    for name, kw in (("loudness_half_life", dict(half_life=0)), ("loudness_half_life", dict(half_life=True)),
                     ("loudness_prior", dict(prior=-1)), ("loudness_prior", dict(prior="1")),
                     ("loudness_gate_lufs", dict(gate_lufs=-10)), ("loudness_gate_lufs", dict(gate_lufs=float("nan"))),
                     ("loudness_max_db", dict(max_db=-1)), ("loudness_slew_db", dict(slew_db=0)),
                     ("loudness_slew_db", dict(slew_db=float("inf")))):
        with pytest.raises(ValueError, match=name + "="):
            MS.check_loudness_stream(**kw)


# ------------------------------------------------------------------------------------------------ the settings
def _host_converter(loud, rates=None, osr=16000):
    """the part of a converter the loudness validation reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.loud, c.chunk, c.buffersize, c.input_sr, c.output_sr = loud, 160, 16, 16000, osr
    c._rt, c.rate = None, [16000, 16000, 44100]
    c._loud = MS.check_loudness_stream()
    if rates:
        c._rt, c._chunks = object(), {16000: 160, 44100: 441, 48000: 480}
    return c


def test_session_loudness_is_checked_against_the_converter():
    assert "lufs" in MS._PARAMS
    on, off, multi = _host_converter(True), _host_converter(False), _host_converter(True, rates=True)
    assert on._session_loudness(0, {}) == (False, 0, None, None) == off._session_loudness(1, dict(lufs=None))
    ok, hop, coef, par = on._session_loudness(0, dict(lufs=-20))
    assert ok is True and hop == 1600 and np.array_equal(np.array(coef), R.coefficients(16000))
    assert np.array_equal(np.array(par), R.params(16000, 160, -20.0))
    ok, hop, coef, par = multi._session_loudness(2, dict(lufs=-16))             # the slot's own rate: 440 of 441 samples emitted
    assert hop == 4410 and np.array_equal(np.array(coef), R.coefficients(44100))
    assert np.array_equal(np.array(par), R.params(44100, 440, -16.0))
    assert multi._session_loudness(0, dict(lufs=-16), 48000)[1] == 4800         # open(): the rate the slot is about to take
    up = _host_converter(True, osr=48000)                                       # input_sr != output_sr: the output wave's rate
    ok, hop, coef, par = up._session_loudness(0, dict(lufs=-23))
    assert hop == 4800 and np.array_equal(np.array(par), R.params(48000, 160, -23.0))
    with pytest.raises(ValueError, match=r"slot 2: lufs=-23 needs a converter built with MultiStreamConverter\(..., loudness=True\)"):
        off._session_loudness(2, dict(lufs=-23))
    for bad in ("5", True, float("nan"), 1, -70):
        for conv in (on, off):
            with pytest.raises(ValueError, match="slot 1: lufs=.* must be a finite number of LUFS"):
                conv._session_loudness(1, dict(lufs=bad))
    with pytest.raises(ValueError, match="loudness must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, loudness=1)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: loudness_half_life=0 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, loudness=True, loudness_half_life=0)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: loudness_slew_db=-1 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, loudness=True, loudness_slew_db=-1)
    with pytest.raises(ValueError, match=r"loudness needs a converter built with MultiStreamConverter\(..., loudness=True\)"):
        off.loudness()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_loudness_symbols_are_exported_and_the_prototypes_agree_with_the_header():
    L = ctypes.CDLL(nat.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    kind = lambda a: (ctypes.c_void_p if "*" in a else ctypes.c_double if "double" in a else                      # noqa: E731
                      ctypes.c_size_t if "size_t" in a else ctypes.c_int)
    for name, res, nargs in (("alive_loudness_workspace_bytes", "size_t", 2), ("alive_loudness_measure_waves", "int", 15),
                             ("alive_loudness_apply_waves", "int", 11), ("alive_loudness_rows", "int", 12)):
        assert hasattr(L, name)
        decl = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl is not None, f"{name} is not declared in alive_vc.h"
        args = decl.group(1).split(",")
        assert len(args) == nargs == len(nat.PROTOTYPES[name][1])
        assert nat.PROTOTYPES[name][0] is (ctypes.c_size_t if res == "size_t" else ctypes.c_int)
        assert [kind(a) for a in args] == nat.PROTOTYPES[name][1], name
    mk = open(os.path.join(ROOT, "alive-vc_amd", "csrc", "Makefile")).read()
    assert "loudness.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]
    assert "-ffp-contract=off" in mk and "-fno-fast-math" in mk and "-ffast-math" not in mk.replace("-fno-fast-math", "")


def test_loudness_abi_refuses_bad_arguments():
    L = nat.lib()
    assert L.alive_loudness_workspace_bytes(3, 100) == 3 * 100 * 9 * 8
    for bad in ((0, 10), (-1, 10), (65536, 10), (4, 0), (4, -2)):
        assert L.alive_loudness_workspace_bytes(*bad) == 0
    #     y   N  ld  len hop coef ap  z_abs  tiles zI  c1  c2  ws  bytes     stream
    ok = [16, 2, 64, 16, 16, 16,  16, 1e-7,  4,    16, 16, 16, 16, 2 * 4 * 72, None]
    for i in (0, 3, 4, 5, 6, 9, 10, 11, 12):
        a = list(ok)
        a[i] = None
        assert L.alive_loudness_measure_waves(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((1, 0), (1, -1), (1, 65536), (2, 0), (2, -5), (8, 0), (8, -1), (7, 0.0), (7, -1.0), (7, float("nan")),
                   (7, float("inf"))):
        a = list(ok)
        a[i] = bad
        assert L.alive_loudness_measure_waves(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)
    a = list(ok)
    a[13] -= 1
    assert L.alive_loudness_measure_waves(*a) == -1 and b"workspace" in L.alive_last_error()
    #     out    y     N  ld  len zI  c2  z_t gmax gain  stream
    ok = [4096, 8192, 2, 64, 16, 16, 16, 16, 4.0, None, None]
    for i in (0, 1, 4, 5, 6, 7):
        a = list(ok)
        a[i] = None
        assert L.alive_loudness_apply_waves(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((2, 0), (2, -1), (2, 65536), (3, 0), (3, -2), (8, 0.5), (8, float("nan")), (8, float("inf"))):
        a = list(ok)
        a[i] = bad
        assert L.alive_loudness_apply_waves(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)
    for out, y in ((8192, 8192), (8192 + 4, 8192), (8192 - 2 * 64 * 4 + 4, 8192), (8192 + 2 * 64 * 4 - 4, 8192)):
        a = list(ok)
        a[0], a[1] = out, y
        assert L.alive_loudness_apply_waves(*a) == -1 and b"overlaps" in L.alive_last_error(), (out, y)
    #     y   N  ld  lo  len emit on  hop coef par state stream
    ok = [16, 2, 64, 16, 16, 16,  16, 16, 16,  16,  16,   None]
    for i in (0, 3, 4, 5, 6, 7, 8, 9, 10):
        a = list(ok)
        a[i] = None
        assert L.alive_loudness_rows(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((1, 0), (1, -1), (2, 0), (2, -5)):
        a = list(ok)
        a[i] = bad
        assert L.alive_loudness_rows(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)


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


def test_sessions_file_takes_a_loudness_target_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    assert MSI.LOUDNESS_KEYS == ("lufs",)
    a, b = MSI.load_sessions(write(files, [sess, dict(sess, lufs=-23)]))
    assert "lufs" not in a and set(a) == set(MSI.SESSION_KEYS) and b["lufs"] == -23.0 and isinstance(b["lufs"], float)
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, lufs=None), dict(sess, lufs=-16)]), lufs=-20)
    assert (a["lufs"], b.get("lufs"), c["lufs"]) == (-20.0, None, -16.0) and "lufs" not in b
    for bad in ("-23", True, [1], 2, -70, -80):
        with pytest.raises(ValueError, match=r"session 1: lufs="):
            MSI.load_sessions(write(files, [sess, dict(sess, lufs=bad)]))
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['loudness'\]"):
        MSI.load_sessions(write(files, [dict(sess, loudness=-23)]))
    with pytest.raises(ValueError, match=r"-lufs: lufs=3 must be"):
        MSI.load_sessions(write(files, [sess]), lufs=3)
    p = MSI.build_parser()
    args = p.parse_args(["s.json"])
    assert (args.lufs, args.loudness_half_life, args.loudness_prior, args.loudness_gate, args.loudness_max_db,
            args.loudness_slew) == (None, 3.0, 1.0, -70.0, 12.0, 6.0)
    args = p.parse_args(["s.json", "-lufs", "-16", "--loudness-half-life", "2", "--loudness-prior", "0.5", "--loudness-gate", "-60",
                         "--loudness-max-db", "6", "--loudness-slew", "3"])
    assert (args.lufs, args.loudness_half_life, args.loudness_prior, args.loudness_gate, args.loudness_max_db,
            args.loudness_slew) == (-16.0, 2.0, 0.5, -60.0, 6.0, 3.0)


def test_jobs_file_takes_a_loudness_target_per_job(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    assert BI.LOUDNESS_KEYS == ("lufs",)
    a, b = BI.load_jobs(write(files, [job, dict(job, lufs=-23)]))
    assert "lufs" not in a and set(a) == set(BI.JOB_KEYS) and b["lufs"] == -23.0 and set(b) == set(BI.JOB_KEYS + BI.LOUDNESS_KEYS)
    a, b, c = BI.load_jobs(write(files, [job, dict(job, lufs=None), dict(job, lufs=-16)]), lufs=-20)
    assert (a["lufs"], b.get("lufs"), c["lufs"]) == (-20.0, None, -16.0) and "lufs" not in b
    for bad in ("-1", True, 2, float("nan"), -70):
        with pytest.raises(ValueError, match=r"job 1: lufs="):
            BI.load_jobs(write(files, [job, dict(job, lufs=bad)]))
    with pytest.raises(ValueError, match=r"-lufs / --loudness-max-db: loudness max gain -1 must be"):
        BI.load_jobs(write(files, [job]), loudness_max_db=-1)
    with pytest.raises(ValueError, match=r"job 0: unknown keys \['loudness_max_db'\]"):
        BI.load_jobs(write(files, [dict(job, loudness_max_db=3)]))
    args = BI.build_parser().parse_args(["j.json"])
    assert (args.lufs, args.loudness_max_db) == (None, 12.0)
    args = BI.build_parser().parse_args(["j.json", "-lufs", "-23", "--loudness-max-db", "20"])
    assert (args.lufs, args.loudness_max_db) == (-23.0, 20.0)


def test_inference_takes_the_loudness_flags():
    import inference as INF
    args = INF.build_parser().parse_args([])
    assert (args.lufs, args.loudness_max_db) == (None, 12.0)
    args = INF.build_parser().parse_args(["-lufs", "-16", "--loudness-max-db", "6"])
    assert (args.lufs, args.loudness_max_db) == (-16.0, 6.0)
