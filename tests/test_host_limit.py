"""CPU tests of the output limiter: the NumPy restatement tools/limit_ref.py (the bound on peaky input, a quiet signal bitwise, stream
equals offline bitwise with a consistent continuation -- an odd chunk included --, the bound under a wrong continuation, non-finite
samples), limit_geometry / check_limit / limit_history_width with every refusal and the largest value that fits, the validation on
converters without a device, the sessions and jobs files, the CLIs' flags, and the C ABI (symbols, prototypes, refusals)."""
import ctypes
import json
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
import limit_ref as LR                                               # noqa: E402
import batch_inference as BI                                         # noqa: E402
import multistream_inference as MSI                                  # noqa: E402

C1 = np.float32(10.0 ** (-1.0 / 20.0))                               # -1 dBFS


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def _peaky(n, seed, scale=0.5, peaks=12, height=4.0):
    """noise well under the ceiling with a few samples far above it"""
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(n) * scale * 0.3).astype(np.float32)
    at = rng.choice(n, peaks, replace=False)
    y[at] = (rng.uniform(1.0, height, peaks) * rng.choice([-1.0, 1.0], peaks)).astype(np.float32)
    return y


# ------------------------------------------------------------------------------------------------ the restatement
def test_no_sample_exceeds_the_ceiling_on_peaky_input():
    for seed, (L, H), c in ((0, (80, 160), C1), (1, (1, 0), np.float32(0.5)), (2, (7, 0), LR.CEIL_MAX), (3, (2, 33), np.float32(0.1))):
        y = _peaky(3000, seed)[None]
        out, gmin = LR.limit_waves(y, [3000], L, H, [c])
        assert np.abs(y).max() > 1.0 and np.abs(out).max() <= c and out.dtype == np.float32
        assert 0 < gmin[0] < 1 and np.isfinite(out).all()
        # the gain is the required one where the peak is, and never above it anywhere
        a = LR.required(y[0], c)
        with np.errstate(invalid="ignore", divide="ignore"):
            g_eff = np.where(y[0] != 0, out[0] / y[0], 1.0)
        assert np.all(g_eff <= a * (1 + 2e-7))
    assert float(LR.CEIL_MAX) * 32768 == 32767.0


def test_the_gain_ramps_down_before_a_peak_holds_and_ramps_back():
    L, H, n, at = 8, 5, 80, 40
    y = np.full(n, 0.25, np.float32)
    y[at] = 2.0
    a = np.concatenate([np.ones(L - 1 + H, np.float32), LR.required(y, 0.5), np.ones(L - 1, np.float32)])
    g = LR.gains(a, L, H, n)
    assert np.all(g[:at - L + 1] == 1.0) and np.all(g[at + H + L:] == 1.0)
    assert np.all(np.diff(g[at - L:at + 1]) < 0)                     # the ramp down: L steps, the first L - 1 samples ahead of the peak
    assert np.all(g[at:at + H + 1] == np.float32(0.25))              # down as the peak arrives, held for H after it
    assert np.all(np.diff(g[at + H:at + H + L + 1]) > 0)             # the ramp back: L steps
    assert LR.apply(y, g, 0.5)[at] == np.float32(0.5)


def test_a_quiet_signal_comes_back_bitwise():
    rng = np.random.default_rng(5)
    y = (rng.uniform(-1, 1, (2, 1500)) * C1).astype(np.float32)
    y[0, 7], y[1, 9], y[0, 11], y[1, 13] = C1, -C1, 0.0, -0.0
    out, gmin = LR.limit_waves(y, [1500, 1200], 80, 160, [C1, C1])
    assert np.array_equal(_bits(out), _bits(y)) and gmin.tolist() == [1.0, 1.0]
    hist = np.ones((2, 300), np.float32)
    got, h2, gm = LR.limit_rows(y, [100, 100], [400, 400], [400, 401], [80, 1], [160, 0], [C1, C1], [1, 1], hist)
    assert np.array_equal(_bits(got), _bits(y)) and np.all(h2 == 1.0) and gm.tolist() == [1.0, 1.0]


def _windows(sig, ticks, ld, shift):
    return [sig[t * shift:t * shift + ld][None].copy() for t in range(ticks)]


@pytest.mark.parametrize("geom", [dict(span=160, shift=160, L=80, H=160, ticks=29), dict(span=440, shift=441, L=220, H=300, ticks=9),
                                  dict(span=50, shift=50, L=50, H=210, ticks=30), dict(span=64, shift=64, L=1, H=0, ticks=12)])
def test_stream_equals_offline_bitwise_with_a_consistent_continuation(geom):
    """successive waves are one signal moved on by `shift`, so each tick's lookahead is what the next tick emits.  With an odd chunk
    (shift = span + 1) the emitted stream drops one sample per tick, as the converters do"""
    span, shift, L, H, ticks = (geom[k] for k in ("span", "shift", "L", "H", "ticks"))
    lo, ld, ld_hist = 30, 30 + shift + 2 * span, L - 1 + H + 3
    sig = _peaky(ticks * shift + ld, 7 + span, peaks=40)
    waves = _windows(sig, ticks, ld, shift)
    _, spans, gmins, hist = LR.stream(waves, [lo], [span], [shift], [L], [H], [C1], ld_hist=ld_hist)
    got = np.concatenate([s[0] for s in spans])
    emitted = np.concatenate([w[0, lo:lo + span] for w in waves] + [waves[-1][0, lo + shift:lo + shift + L - 1]])
    want, gmin = LR.limit_waves(emitted[None], [len(emitted)], L, H, [C1])
    assert np.array_equal(_bits(got), _bits(want[0, :ticks * span])) and np.abs(got).max() <= C1 and np.abs(emitted).max() > 1
    assert not np.array_equal(got, emitted[:ticks * span]) and min(float(g[0]) for g in gmins) < 1
    a = LR.required(emitted[:ticks * span], C1)
    assert np.array_equal(_bits(hist[0]), _bits(np.concatenate([np.ones(ld_hist, np.float32), a])[-ld_hist:]))


def test_the_bound_holds_under_a_wrong_continuation():
    span, shift, L, H, ticks, lo = 160, 160, 80, 160, 20, 30
    ld = lo + shift + 2 * span
    sig = _peaky(ticks * shift + ld, 11, peaks=60)
    waves = _windows(sig, ticks, ld, shift)
    right = LR.stream(waves, [lo], [span], [shift], [L], [H], [C1], ld_hist=300)[1]
    for w in waves:
        w[0, lo + shift:] *= np.float32(0.5)                         # every tick predicts a future half as loud as it turns out
    wrong = LR.stream(waves, [lo], [span], [shift], [L], [H], [C1], ld_hist=300)[1]
    got, ref = np.concatenate([s[0] for s in wrong]), np.concatenate([s[0] for s in right])
    assert np.abs(got).max() <= C1 and not np.array_equal(got, ref)


def test_non_finite_samples_do_not_spread():
    y = _peaky(600, 13)[None] * np.float32(0.2)
    y[0, 100], y[0, 300], y[0, 450] = np.nan, np.inf, -np.inf
    L, H = 16, 10
    out, gmin = LR.limit_waves(y, [600], L, H, [C1])
    assert np.isfinite(out).all() and np.abs(out).max() <= C1
    assert out[0, 100] == -C1 and out[0, 300] == -C1 and out[0, 450] == -C1          # NaN, and inf * 0 = NaN: fmin(fmax(NaN, -c), c)
    assert gmin[0] == 0.0 and LR.gain_db(gmin)[0] == -np.inf
    a = LR.required(y[0], C1)
    assert a[100] == 1.0 and a[300] == 0.0 and a[450] == 0.0
    # a NaN asks for nothing: its neighbours are untouched; an inf drives its neighbours' gain towards 0, within L + H only
    assert np.array_equal(_bits(out[0, 60:100]), _bits(y[0, 60:100])) and np.array_equal(_bits(out[0, 101:140]), _bits(y[0, 101:140]))
    assert np.all(np.abs(out[0, 300 - L + 1:300]) <= np.abs(y[0, 300 - L + 1:300])) and np.all(out[0, 301:301 + H] == 0.0)
    far = np.r_[0:300 - L + 1, 300 + H + L:450 - L + 1, 450 + H + L:600]
    far = far[far != 100]
    assert np.array_equal(_bits(out[0, far]), _bits(y[0, far]))


def test_rows_that_are_filling_off_or_do_not_fit():
    rng = np.random.default_rng(17)
    ld, ld_hist = 200, 130
    y = (rng.standard_normal((11, ld)) * 2).astype(np.float32)
    hist = rng.uniform(0.2, 1, (11, ld_hist)).astype(np.float32)
    #       filling off  lo<0 span>shift L>shift past-row P>hist c=0  c>1  fits-exactly fits
    lo = [10,    10,  -1,  10,        10,     82,      10,    10,  10,  81,          0]
    span = [50,  50,  50,  61,        50,     50,      50,    50,  50,  50,          50]
    sh = [60,    60,  60,  60,        10,     60,      60,    60,  60,  60,          50]
    L = [8,      0,   8,   8,         11,     60,      8,     8,   8,   60,          8]
    H = [4,      4,   4,   4,         0,      0,       124,   4,   4,   0,           123]
    c = [0.5,    0.5, 0.5, 0.5,       0.5,    0.5,     0.5,   0.0, 1.5, 0.5,         0.5]
    ld_hist_big, hist_big = ld_hist, hist
    emit = [0] + [1] * 10
    got, h2, gm = LR.limit_rows(y, lo, span, sh, L, H, c, emit, hist_big)
    assert np.array_equal(got[:9], y[:9]) and np.array_equal(h2[0], hist_big[0]) and np.all(h2[1:9] == 1.0)
    assert np.isnan(gm[0]) and gm[1:9].tolist() == [1.0] * 8
    assert [LR.fits(a, b, s, l, h, ld, ld_hist_big) for a, b, s, l, h in zip(lo, span, sh, L, H)] == [
        True, False, False, False, False, False, False, True, True, True, True]
    for r in (9, 10):
        assert not np.array_equal(got[r], y[r]) and np.abs(got[r, lo[r]:lo[r] + span[r]]).max() <= 0.5 and gm[r] < 1
        assert np.array_equal(got[r, :lo[r]], y[r, :lo[r]]) and np.array_equal(got[r, lo[r] + span[r]:], y[r, lo[r] + span[r]:])
        assert np.array_equal(h2[r, -span[r]:], LR.required(y[r, lo[r]:lo[r] + span[r]], 0.5))
        assert np.array_equal(h2[r, :-span[r]], hist_big[r, span[r]:])


# ------------------------------------------------------------------------------------------------ the parameter helper
def test_check_limit_values_and_refusals():
    c, look, hold = MS.check_limit(-1.0, 5, 20)
    assert abs(c - 10 ** -0.05) < 1e-15 and (look, hold) == (5.0, 20.0) and isinstance(look, float)
    assert MS.check_limit(0, 5, 0)[0] == 32767 / 32768 == MS.LIMIT_CEIL_MAX and MS.check_limit(-0.0001, 1, 1)[0] == 32767 / 32768
    assert MS.check_limit(None) is None and MS.check_limit(np.float32(-6), np.int64(2), np.float64(0))[0] == 10 ** -0.3
    for bad in ("-1", True, False, [1], float("nan"), float("-inf"), 0.5, 3):
        with pytest.raises(ValueError, match=r"limit_db=.* must be a finite number of dBFS <= 0, or None for no limiter"):
            MS.check_limit(bad)
    for bad in ("5", True, None, float("nan"), float("inf"), 0, -1):
        with pytest.raises(ValueError, match=r"limit_lookahead_ms=.* must be a finite number of milliseconds > 0"):
            MS.check_limit(-1, bad, 20)
        with pytest.raises(ValueError, match=r"limit_lookahead_ms="):      # checked even where the limiter is off
            MS.check_limit(None, bad, 20)
    for bad in ("5", True, None, float("nan"), float("inf"), -1):
        with pytest.raises(ValueError, match=r"limit_hold_ms=.* must be a finite number of milliseconds >= 0"):
            MS.check_limit(-1, 5, bad)
    assert MS.limit_samples(5, 20, 16000) == (80, 320) and MS.limit_samples(5, 20, 44100) == (220, 882)
    assert MS.limit_samples(0.01, 0, 16000) == (1, 0) and MS.limit_samples(5, 20, 48000) == (240, 960)


def test_limit_geometry_values():
    c = 10 ** -0.05
    assert MS.limit_geometry(160, 16, 16000, -1, 5, 20, 2560, 800) == (1200, 160, 80, 320, c)
    assert MS.limit_geometry(441, 16, 44100, -1, 5, 20, 7056, 2400) == (3308, 441, 220, 882, c)      # shift 441, span 440
    assert MS.limit_geometry(480, 16, 48000, -1, 5, 20, 7680, 2400) == (3600, 480, 240, 960, c)
    assert MS.limit_geometry(480, 16, 48000, None, 5, 20, 7680, 2400) == (3600, 480, 0, 0, 1.0)
    assert MS.limit_geometry(160, 16, 16000, 0, 10, 0, 2560, 159) == (1200, 160, 160, 0, 32767 / 32768)       # P = ld_hist exactly
    assert MS.limit_geometry(160, 16, 16000, -1, 5, 45.0625, 2560, 800)[2:4] == (80, 721)                  # L - 1 + H = 800
    assert MS.limit_geometry(160, 16, 16000, -1, 5, 20, 1439, 800)[2] == 80                                # 1200 + 160 + 79 = 1439
    assert MS.limit_geometry(960, 8, 48000, -1, 5, 20, 23040, 2400, shift=2880) == (3360, 2880, 240, 960, c)


def test_limit_geometry_refusals_name_the_largest_value_that_fits():
    with pytest.raises(ValueError, match=r"limit_lookahead_ms=11 is 176 samples at 16000 Hz; a session with 160-sample chunks in a wave "
                                         r"of 2560 and a history of 800 takes 1 to 160 \(the largest limit_lookahead_ms that fits is 10\)"):
        MS.limit_geometry(160, 16, 16000, -1, 11, 20, 2560, 800)
    with pytest.raises(ValueError, match=r"limit_lookahead_ms=5 is 80 samples.*in a wave of 1438 and a history of 800 takes 1 to 79 \(the "
                                         r"largest limit_lookahead_ms that fits is 4.9375\)"):
        MS.limit_geometry(160, 16, 16000, -1, 5, 20, 1438, 800)
    with pytest.raises(ValueError, match=r"takes 1 to 0 \(the largest limit_lookahead_ms that fits is 0\)"):
        MS.limit_geometry(160, 16, 16000, -1, 5, 20, 1300, 800)
    with pytest.raises(ValueError, match=r"limit_lookahead_ms=5 is 80 samples.*a history of 50 takes 1 to 51 \(the largest "
                                         r"limit_lookahead_ms that fits is 3.1875\)"):
        MS.limit_geometry(160, 16, 16000, -1, 5, 0, 2560, 50)
    with pytest.raises(ValueError, match=r"limit_hold_ms=60 is 960 samples at 16000 Hz; beside a lookahead of 80 a history of 800 takes "
                                         r"0 to 721 \(the largest limit_hold_ms that fits is 45.0625\)"):
        MS.limit_geometry(160, 16, 16000, -1, 5, 60, 2560, 800)
    with pytest.raises(ValueError, match=r"limit_hold_ms=20 is 882 samples at 44100 Hz; beside a lookahead of 220 a history of 800 "
                                         r"takes 0 to 581"):
        MS.limit_geometry(441, 16, 44100, -1, 5, 20, 7056, 800)
    with pytest.raises(ValueError, match=r"limit_db=1 must be a finite number of dBFS <= 0"):
        MS.limit_geometry(160, 16, 16000, 1, 5, 20, 2560, 800)


def test_limit_history_width():
    assert MS.limit_history_width(0.05, 48000) == 2400 and MS.limit_history_width(0.05, 16000) == 800
    assert MS.limit_history_width(0.064, 48000) == 3072 == MS.LIMIT_MAX_HIST
    for bad in ("1", True, None, float("nan"), 0, -1):
        with pytest.raises(ValueError, match=r"limit_history=.* must be a finite number of seconds > 0"):
            MS.limit_history_width(bad, 16000)
    with pytest.raises(ValueError, match=r"limit_history=0.1 is 4800 samples at 48000 Hz; the limiter keeps 1 to 3072 \(the largest "
                                         r"limit_history that fits is 0.064\)"):
        MS.limit_history_width(0.1, 48000)
    with pytest.raises(ValueError, match=r"limit_history=1e-06 is 0 samples"):
        MS.limit_history_width(1e-6, 16000)
    hdr = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    assert int(re.search(r"#define ALIVE_LIMIT_TILE (\d+)", hdr).group(1)) == MS.LIMIT_TILE
    assert int(re.search(r"#define ALIVE_LIMIT_MAX_HIST (\d+)", hdr).group(1)) == MS.LIMIT_MAX_HIST
    assert MS.gmin_db([1.0, 0.5, 0.0]) == [0.0, 20 * np.log10(0.5), -np.inf]


# ------------------------------------------------------------------------------------------------ the settings
class _Hist:
    def __init__(self, width):
        self.shape = (1, width)


def _host_converter(limiter, rates=None, osr=16000):
    """the part of a converter the limiter's validation reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.limiter, c.chunk, c.buffersize, c.input_sr, c.output_sr = limiter, 160, 16, 16000, osr
    c._rt, c.rate = None, [16000, 16000, 44100]
    c._limit_len = {16000: 2560 * osr // 16000}
    c.limit_hist = _Hist(800 * osr // 16000)
    if rates:
        c._rt, c._chunks, c._limit_len = object(), {16000: 160, 44100: 441, 48000: 480}, {16000: 2560, 44100: 7056, 48000: 7680}
        c.limit_hist = _Hist(2400)
    return c


def test_session_limiter_is_checked_against_the_converter():
    assert all(k in MS._PARAMS for k in ("limit_db", "limit_lookahead_ms", "limit_hold_ms"))
    on, off, multi = _host_converter(True), _host_converter(False), _host_converter(True, rates=True)
    c = 10 ** -0.05
    assert on._session_limit(0, dict(limit_db=-1)) == (80, 320, c)
    assert on._session_limit(0, dict(limit_db=-1, limit_lookahead_ms=10, limit_hold_ms=0)) == (160, 0, c)
    assert on._session_limit(0, dict(limit_db=None)) == (0, 0, 1.0) == on._session_limit(0, {}) == off._session_limit(1, {})
    assert multi._session_limit(2, dict(limit_db=-1)) == (220, 882, c)                    # the slot's own rate, 44.1 kHz
    assert multi._session_limit(0, dict(limit_db=-1), 48000) == (240, 960, c)             # open(): the rate the slot is about to take
    with pytest.raises(ValueError, match=r"slot 2: limit_db=-1 needs a converter built with MultiStreamConverter\(..., limiter=True\)"):
        off._session_limit(2, dict(limit_db=-1))
    for bad in ("5", True, float("nan"), 1):
        for conv in (on, off):
            with pytest.raises(ValueError, match="slot 1: limit_db=.* must be a finite number of dBFS <= 0"):
                conv._session_limit(1, dict(limit_db=bad))
    with pytest.raises(ValueError, match=r"slot 1: limit_lookahead_ms=11 is 176 samples at 16000 Hz.*that fits is 10\)"):
        on._session_limit(1, dict(limit_db=-1, limit_lookahead_ms=11))
    with pytest.raises(ValueError, match=r"slot 1: limit_hold_ms=60 is 960 samples.*that fits is 45.0625\)"):
        on._session_limit(1, dict(limit_db=-1, limit_hold_ms=60))
    with pytest.raises(ValueError, match=r"slot 0: limit_hold_ms=-1 must be"):
        off._session_limit(0, dict(limit_hold_ms=-1))
    # input_sr != output_sr: L and H in samples of the output wave, the lookahead one tick's advance on at the output rate
    up = _host_converter(True, osr=48000)
    assert up._limit_shift(160) == 480 and on._limit_shift(160) == 160 and _host_converter(True, osr=8000)._limit_shift(160) == 160
    assert up._session_limit(0, dict(limit_db=-1, limit_lookahead_ms=2)) == (96, 960, c)
    with pytest.raises(ValueError, match="limiter must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, limiter=1)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: limit_history=0.1 is 4800 samples at 48000 Hz"):
        MS.MultiStreamConverter(None, None, None, None, 1, limiter=True, limit_history=0.1, rates=[48000])
    with pytest.raises(ValueError, match=r"limit_db needs a converter built with MultiStreamConverter\(..., limiter=True\)"):
        off.limit_db()


def test_realtime_converter_checks_its_limiter_before_anything_is_built():
    from module.realtime import RealtimeConverter
    for bad in ("5", True, 1, float("nan")):
        with pytest.raises(ValueError, match="limit_db=.* must be a finite number of dBFS <= 0"):
            RealtimeConverter(None, None, None, None, limit_db=bad)
    with pytest.raises(ValueError, match="limit_lookahead_ms=0 must be"):
        RealtimeConverter(None, None, None, None, limit_db=-1, limit_lookahead_ms=0)
    with pytest.raises(ValueError, match=r"limit_history=1 is 16000 samples at 16000 Hz"):
        RealtimeConverter(None, None, None, None, limit_db=-1, limit_history=1)
    rt = RealtimeConverter.__new__(RealtimeConverter)
    assert rt.limiter is False
    with pytest.raises(ValueError, match=r"limit_db needs a converter built with RealtimeConverter\(..., limit_db=DB\)"):
        rt.limit_db()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_limiter_symbols_are_exported_and_the_prototypes_agree_with_the_header():
    L = ctypes.CDLL(nat.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    for name, nargs in (("alive_limit_rows", 14), ("alive_limit_waves", 10)):
        assert hasattr(L, name)
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl is not None, f"{name} is not declared in alive_vc.h"
        assert len(decl.group(1).split(",")) == nargs == len(nat.PROTOTYPES[name][1]) and nat.PROTOTYPES[name][0] is ctypes.c_int
        kinds = [ctypes.c_void_p if "*" in a else ctypes.c_int for a in decl.group(1).split(",")]
        assert kinds == nat.PROTOTYPES[name][1], name
    mk = open(os.path.join(ROOT, "alive-vc_amd", "csrc", "Makefile")).read()
    assert "limit.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]
    assert "-ffp-contract=off" in mk and "-fno-fast-math" in mk and "-ffast-math" not in mk.replace("-fno-fast-math", "")


def test_limit_abi_refuses_bad_arguments():
    L = nat.lib()
    #     y   N  ld  lo  span shift look hold ceil emit hist ld_hist gmin  stream
    ok = [16, 2, 64, 16, 16,  16,   16,  16,  16,  16,  16,  8,      None, None]
    for i in (0, 3, 4, 5, 6, 7, 8, 9, 10):
        a = list(ok)
        a[i] = None
        assert L.alive_limit_rows(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((1, 0), (1, -1), (2, 0), (2, -5), (11, 0), (11, -1), (11, MS.LIMIT_MAX_HIST + 1)):
        a = list(ok)
        a[i] = bad
        assert L.alive_limit_rows(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)
    #     out    y     N  ld  len look hold ceil gmin  stream
    ok = [4096, 8192, 2, 64, 16,  8,   4,   16,  None, None]
    for i in (0, 1, 4, 7):
        a = list(ok)
        a[i] = None
        assert L.alive_limit_waves(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((2, 0), (2, -1), (2, 65536), (3, 0), (3, -2), (5, 0), (5, -1), (6, -1), (5, MS.LIMIT_MAX_HIST + 2),
                   (6, MS.LIMIT_MAX_HIST - 6)):
        a = list(ok)
        a[i] = bad
        assert L.alive_limit_waves(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)
    for out, y in ((8192, 8192), (8192 + 4, 8192), (8192 - 2 * 64 * 4 + 4, 8192), (8192 + 2 * 64 * 4 - 4, 8192)):
        a = list(ok)
        a[0], a[1] = out, y
        assert L.alive_limit_waves(*a) == -1 and b"overlaps" in L.alive_last_error(), (out, y)


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


def test_sessions_file_takes_a_limiter_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, limit_db=-1), dict(sess, limit_db=-3, limit_lookahead_ms=2,
                                                                                  limit_hold_ms=0)]))
    assert not set(a) & set(MSI.LIMIT_KEYS) and set(a) == set(MSI.SESSION_KEYS)
    assert (b["limit_db"], b["limit_lookahead_ms"], b["limit_hold_ms"]) == (-1.0, 5.0, 20.0)
    assert (c["limit_db"], c["limit_lookahead_ms"], c["limit_hold_ms"]) == (-3.0, 2.0, 0.0) and isinstance(c["limit_db"], float)
    # -lim and the two --limit-* flags are the defaults; a session's null switches the limiter off, its own values win
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, limit_db=None), dict(sess, limit_db=-6, limit_hold_ms=7)]),
                                limit_db=-2, limit_lookahead_ms=3, limit_hold_ms=11)
    assert (a["limit_db"], a["limit_lookahead_ms"], a["limit_hold_ms"]) == (-2.0, 3.0, 11.0) and "limit_db" not in b
    assert (c["limit_db"], c["limit_lookahead_ms"], c["limit_hold_ms"]) == (-6.0, 3.0, 7.0)
    for bad in ("-1", True, [1], 2):
        with pytest.raises(ValueError, match=r"session 1: limit_db="):
            MSI.load_sessions(write(files, [sess, dict(sess, limit_db=bad)]))
    with pytest.raises(ValueError, match=r"session 0: limit_lookahead_ms=0 must be"):
        MSI.load_sessions(write(files, [dict(sess, limit_lookahead_ms=0)]))
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['limit'\]"):
        MSI.load_sessions(write(files, [dict(sess, limit=-1)]))
    with pytest.raises(ValueError, match=r"-lim / --limit-lookahead / --limit-hold: limit_db=3 must be"):
        MSI.load_sessions(write(files, [sess]), limit_db=3)
    with pytest.raises(ValueError, match=r"-lim / --limit-lookahead / --limit-hold: limit_hold_ms=-1 must be"):
        MSI.load_sessions(write(files, [sess]), limit_hold_ms=-1)
    p = MSI.build_parser()
    args = p.parse_args(["s.json"])
    assert (args.limit, args.limit_lookahead, args.limit_hold) == (None, 5.0, 20.0)
    args = p.parse_args(["s.json", "-lim", "-1.5", "--limit-lookahead", "2", "--limit-hold", "0"])
    assert (args.limit, args.limit_lookahead, args.limit_hold) == (-1.5, 2.0, 0.0)


def test_jobs_file_takes_a_limit_per_job(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    assert BI.LIMIT_KEYS == ("limit_db",)
    a, b = BI.load_jobs(write(files, [job, dict(job, limit_db=-1)]))
    assert "limit_db" not in a and set(a) == set(BI.JOB_KEYS) and b["limit_db"] == -1.0 and set(b) == set(BI.JOB_KEYS + BI.LIMIT_KEYS)
    a, b, c = BI.load_jobs(write(files, [job, dict(job, limit_db=None), dict(job, limit_db=-6)]), limit_db=-2)
    assert (a["limit_db"], b.get("limit_db"), c["limit_db"]) == (-2.0, None, -6.0) and "limit_db" not in b
    for bad in ("-1", True, 2, float("nan")):
        with pytest.raises(ValueError, match=r"job 1: limit_db="):
            BI.load_jobs(write(files, [job, dict(job, limit_db=bad)]))
    with pytest.raises(ValueError, match=r"-lim / --limit-lookahead / --limit-hold: limit_lookahead_ms=0 must be"):
        BI.load_jobs(write(files, [job]), lookahead_ms=0)
    with pytest.raises(ValueError, match=r"job 0: unknown keys \['limit_hold_ms'\]"):
        BI.load_jobs(write(files, [dict(job, limit_hold_ms=3)]))
    args = BI.build_parser().parse_args(["j.json"])
    assert (args.limit, args.limit_lookahead, args.limit_hold) == (None, 5.0, 20.0)
    assert BI.build_parser().parse_args(["j.json", "-lim", "-3"]).limit == -3.0


def test_the_other_clis_take_the_limiter():
    import inference as INF
    import realtime_inference as RI
    for mod, argv in ((INF, []), (RI, [])):
        args = mod.build_parser().parse_args(argv)
        assert (args.limit, args.limit_lookahead, args.limit_hold) == (None, 5.0, 20.0)
        args = mod.build_parser().parse_args(["-lim", "-1", "--limit-lookahead", "2.5", "--limit-hold", "10"])
        assert (args.limit, args.limit_lookahead, args.limit_hold) == (-1.0, 2.5, 10.0)
