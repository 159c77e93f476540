"""CPU tests of the post filter: the NumPy restatement tools/postfilter_ref.py (copied rows, silence, the table builders, the size of the
integer sums, the truncation to 128 taps, the level, the effect on a synthetic vowel and the absence of one on noise), check_post_filter
with every refusal, the validation on converters without a device, the sessions and jobs files, the flags of all four CLIs, and the C ABI
(symbol, prototype, refusals).

The figures in the comments were measured with the committed restatement at its defaults (hop 320, window 640, order 16, ratio 0.625,
tilt 0.5, floor -100 dB, range +-12 dB); no bound had to be widened."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from module import _native as nat
from module import multistream as MS
from module import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "alive-vc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import postfilter_ref as PR                                          # noqa: E402
import batch_inference as BI                                         # noqa: E402
import multistream_inference as MSI                                  # noqa: E402

N = 9600


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def _noise(n, seed, scale=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def _rms(v):
    return float(np.sqrt(np.mean(np.asarray(v, dtype=np.float64) ** 2)))


@pytest.fixture(scope="module")
def signals():
    return dict(voiced=synthetic.make_voiced(N, 3)[0][0].numpy(), waveform=synthetic.make_waveform(N, 2)[0].numpy(), noise=_noise(N, 1))


@pytest.fixture(scope="module")
def vowel():
    """an AR(4) vowel: resonators at 700 Hz (130 Hz wide) and 1800 Hz (200 Hz wide), a pulse every 128 samples plus 0.01 N(0, 1),
    peak 0.2"""
    x = np.zeros(N)
    x[::128] = 1.0
    x += 0.01 * np.random.default_rng(11).standard_normal(N)
    a = np.array([1.0])
    for f, bw in ((700.0, 130.0), (1800.0, 200.0)):
        r, th = np.exp(-np.pi * bw / 16000.0), 2 * np.pi * f / 16000.0
        a = np.convolve(a, [1.0, -2 * r * np.cos(th), r * r])
    y = np.zeros(N)
    for i in range(N):
        y[i] = x[i] - sum(a[j] * y[i - j] for j in range(1, 5) if i - j >= 0)
    return (0.2 * y / np.abs(y).max()).astype(np.float32)


def _contrast(v):
    """max - min of the 40-bin-smoothed log power spectrum, Hann-windowed, over bins 40 .. 3040, in dB"""
    p = np.abs(np.fft.rfft(v.astype(np.float64) * np.hanning(len(v)))) ** 2
    s = np.convolve(p, np.ones(40) / 40.0, mode="same")
    level = 10 * np.log10(s[40:3040])
    return float(level.max() - level.min())


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_constants_and_tables_are_those_of_the_python_wrapper():
    assert (PR.TAPS, PR.MAX_ORDER, PR.TILE, PR.HOP) == (MS.POSTFILTER_TAPS, MS.POSTFILTER_MAX_ORDER, MS.POSTFILTER_TILE, MS.POSTFILTER_HOP)
    assert PR.MAX_ALPHA == MS.POSTFILTER_MAX_ALPHA == 0.85
    assert MS.check_post_filter(0.8) == (0.8, PR.RATIO, PR.TILT, PR.ORDER, PR.WINDOW) + PR.constants() == (
        0.8, 0.625, 0.5, 16, 640, 1e-10, 10.0 ** -0.6, 10.0 ** 0.6)
    assert PR.constants(-47.5, 7.25) == MS.check_post_filter(0.3, 0.5, 0.5, 10, 30.0, -47.5, 7.25)[5:]
    for window in (16, 320, 640, 1024):
        assert np.array_equal(PR.window_table(window), MS.postfilter_window(window)) and PR.window_table(window).dtype == np.int16
    for order in (1, 4, 16, 32):
        assert np.array_equal(PR.lag_table(order), MS.postfilter_lag(order)) and PR.lag_table(order).dtype == np.float64
    hdr = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    for name, v in (("TAPS", PR.TAPS), ("MAX_ORDER", PR.MAX_ORDER), ("TILE", PR.TILE)):
        assert f"#define ALIVE_POSTFILTER_{name} {v}\n" in hdr


def test_the_table_builders_against_literal_values():
    assert PR.window_table(16).tolist() == [6, 10, 18, 29, 40, 51, 59, 63, 63, 59, 51, 40, 29, 18, 10, 6]
    w = PR.window_table(640)
    assert w[[0, 1, 159, 319, 320, 639]].tolist() == [5, 5, 34, 64, 64, 5] and w.min() == 5 and w.max() == 64
    assert np.array_equal(w, w[::-1]) and len(w) == 640
    assert PR.lag_table(4).tolist() == [1.0, 0.9997224558987113, 0.9988902856937028, 0.9975048743994922, 0.9955685261050763]
    lag = PR.lag_table(16)
    assert len(lag) == 17 and lag[8] == 0.9823915844707989 and lag[16] == 0.9314049334023056


def test_a_row_outside_the_range_of_alpha_is_copied_bit_for_bit():
    y = _noise((2, 2000), 2)
    y[0, 5], y[0, 6], y[1, 7], y[1, 8] = -0.0, 0.0, np.nan, np.inf
    for bad in (0.0, float("nan"), -0.1, 0.9):
        out, G, mm = PR.postfilter_waves(y, None, bad)
        assert np.array_equal(_bits(out), _bits(y)) and G == [None, None] and mm.tolist() == [[1.0, 1.0]] * 2, bad
    out, G, _ = PR.postfilter_waves(y, [0, -3], 0.8)                  # no samples: copied
    assert np.array_equal(_bits(out), _bits(y)) and G == [None, None]
    out, G, _ = PR.postfilter_waves(y[:1], [700], 0.8)                # samples at or beyond n: copied
    assert np.array_equal(_bits(out[0, 700:]), _bits(y[0, 700:])) and not np.array_equal(out[0, :700], y[0, :700]) and len(G[0]) == 3
    assert PR.filters(0.85, 1) and PR.filters(np.float32(0.85), 1) and not PR.filters(0.8500001, 1) and not PR.filters(0.8, 0)


def test_zeros_stay_zeros_and_take_the_identity():
    z = np.zeros(5 * 320 + 9, np.float32)
    out, g, ident, h = PR.filter_row(z, len(z), 0.8)
    assert not out.any() and np.all(g == 1.0) and ident.all() and np.all(h[:, 0] == 1.0) and not h[:, 1:].any()
    assert np.array_equal(_bits(out), _bits(z)) and PR.postfilter_waves(z[None], None, 0.8)[2].tolist() == [[1.0, 1.0]]


def test_no_frame_of_the_test_signals_takes_the_identity(signals, vowel):
    for name, s in list(signals.items()) + [("vowel", vowel)]:
        _, g, ident, _ = PR.filter_row(s, N, 0.8)
        assert not ident.any() and np.isfinite(g).all(), name


def test_the_integer_sums_stay_below_2_to_the_53_on_a_full_scale_square_wave():
    sq = np.where((np.arange(4096) // 8) % 2 == 0, 1.0, -1.0).astype(np.float32)
    R = PR.autocorrelation(sq, 4096, hop=1024, window=1024, order=32)
    assert R.dtype == np.int64 and np.abs(R).max() < 2 ** 53 and R[:, 0].min() > 2 ** 50       # measured: 1.79e15 against 9.0e15
    assert np.abs(PR.quantise(sq, 4096)).max() == 32767
    # the same sums in fp64 are the same integers: no order can show
    q = PR.quantise(sq, 1024).astype(np.float64) * PR.window_table(1024)
    assert float(np.sum(q * q)) == float(R[0, 0]) == float(np.sum((q * q)[::-1]))


def test_128_taps_are_the_whole_response_at_the_largest_alpha(signals):
    """the output at alpha 0.85 against a 512-tap restatement, before the last rounding: at most 1e-9 of full scale.
    Measured: 5.2e-14 (make_voiced) and 3.5e-11 (make_waveform)"""
    for name in ("voiced", "waveform"):
        a = PR.filter_row(signals[name], N, 0.85, dtype=np.float64)[0]
        b = PR.filter_row(signals[name], N, 0.85, taps=512, dtype=np.float64)[0]
        d = float(np.abs(a - b).max())
        print(f"{name}: 128 against 512 taps {d:.2e}")
        assert d <= 1e-9


@pytest.mark.parametrize("alpha", [0.5, 0.8])
def test_the_level_is_kept(signals, alpha):
    """the RMS of the output within 1 % of the input's.  Measured: 0.004 / 0.018 % (make_voiced), 0.008 / 0.042 % (make_waveform),
    0.021 / 0.14 % (noise) at alpha 0.5 / 0.8"""
    for name, s in signals.items():
        dev = abs(_rms(PR.post_filter(s, alpha)) / _rms(s) - 1.0)
        print(f"{name} at {alpha}: rms off by {100 * dev:.3f} %")
        assert dev <= 0.01, name


def test_the_formants_of_a_vowel_stand_out_more_and_noise_keeps_its_spectrum(vowel, signals):
    """the contrast of the smoothed spectrum rises by at least 2 dB from alpha 0 to 0.5 and again to 0.8 on the vowel (measured:
    82.1 -> 86.6 -> 91.0 dB) and moves by under 0.5 dB on noise at 0.8 (measured: 5.77 -> 5.77)"""
    c = [_contrast(vowel), _contrast(PR.post_filter(vowel, 0.5)), _contrast(PR.post_filter(vowel, 0.8))]
    print("vowel contrast", [round(v, 2) for v in c])
    assert c[1] - c[0] >= 2.0 and c[2] - c[1] >= 2.0
    n0, n1 = _contrast(signals["noise"]), _contrast(PR.post_filter(signals["noise"], 0.8))
    print("noise contrast", round(n0, 2), round(n1, 2))
    assert abs(n1 - n0) < 0.5


def test_a_row_is_the_same_alone_and_stacked():
    n = 9 * 320 + 17
    ys = _noise((4, n), 10, 0.2)
    lens, alphas = [n, 5 * 320, n - 1, 3], [0.8, 0.5, 0.0, 0.85]
    out, G, mm = PR.postfilter_waves(ys, lens, alphas)
    for r in range(4):
        o1, G1, m1 = PR.postfilter_waves(ys[r:r + 1], lens[r:r + 1], alphas[r])
        assert np.array_equal(_bits(o1[0]), _bits(out[r])) and np.array_equal(m1[0], mm[r])
        assert (G1[0] is None and G[r] is None) or np.array_equal(G1[0], G[r])
    o8 = PR.postfilter_waves(ys, lens, alphas, hop=8, window=16, order=4)[0]      # the same function at another frame size
    assert not np.array_equal(o8[0], out[0]) and np.array_equal(_bits(o8[2]), _bits(ys[2]))


def test_non_finite_samples_leave_the_frames_they_reach_at_unity():
    n = 12 * 320
    y = _noise(n, 6, 0.2)
    y[3 * 320 + 300] = np.nan                                        # reaches frames 3 and 4
    y[8 * 320 - 1] = np.inf                                          # the last sample of frame 7: reaches frames 7 and 8
    out, g, ident, _ = PR.filter_row(y, n, 0.8)
    touched = np.zeros(12, bool)
    touched[[3, 4, 7, 8]] = True
    assert np.all(g[touched] == 1.0) and np.all(g[~touched] != 1.0) and not ident.any()
    bad = ~np.isfinite(out)
    assert bad[3 * 320 + 300:3 * 320 + 300 + 128].all() and bad[8 * 320 - 1:8 * 320 + 127].all() and bad.sum() == 256


# ------------------------------------------------------------------------------------------------ the settings
def test_check_post_filter():
    assert MS.check_post_filter(0) == (0.0, 0.625, 0.5, 16, 640, 1e-10, 10.0 ** -0.6, 10.0 ** 0.6)
    assert MS.check_post_filter(np.float32(0.5), 0, 1, np.int64(32), 64, -60, 0)[:5] == (0.5, 0.0, 1.0, 32, 1024)
    assert MS.check_post_filter(0.85, window_ms=20)[4] == 320 and MS.check_post_filter(0.85, window_ms=20.125)[4] == 322
    for bad in (-0.1, 0.86, 1, float("nan"), float("inf"), "0.5", True, None, [0.5]):
        with pytest.raises(ValueError, match=r"post_filter=.* must be a finite number in \[0, 0.85\]"):
            MS.check_post_filter(bad)
    for bad in (-0.1, 1.1, float("nan"), "x", True, None):
        with pytest.raises(ValueError, match="post_filter_ratio=.* must be"):
            MS.check_post_filter(0.5, bad)
        with pytest.raises(ValueError, match="post_filter_tilt=.* must be"):
            MS.check_post_filter(0.5, 0.625, bad)
    for bad in (0, 33, -1, 16.0, True, None, "16"):
        with pytest.raises(ValueError, match=r"post_filter_order=.* must be an integer in \[1, 32\]"):
            MS.check_post_filter(0.5, 0.625, 0.5, bad)
    for bad in (19.875, 64.125, 40.0625, 20.0625, float("nan"), float("inf"), "40", True, None, -40):
        with pytest.raises(ValueError, match="post_filter_window_ms=.* must be"):
            MS.check_post_filter(0.5, 0.625, 0.5, 16, bad)
    for bad in (float("nan"), float("-inf"), "x", True, None, -4000, 4000):
        with pytest.raises(ValueError, match="post_filter_floor_db=.* must be"):
            MS.check_post_filter(0.5, 0.625, 0.5, 16, 40.0, bad)
    for bad in (-1, float("nan"), float("inf"), "6", False, None, 7000):
        with pytest.raises(ValueError, match="post_filter_range_db=.* must be"):
            MS.check_post_filter(0.5, 0.625, 0.5, 16, 40.0, -100.0, bad)


def test_the_offline_call_checks_its_arguments_before_the_device():
    import torch
    y = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match=r"post_filter=0.9 must be"):
        MS.post_filter(y, None, 0.9)
    with pytest.raises(ValueError, match="post_filter_order=40 must be"):
        MS.post_filter(y, None, 0.8, order=40)
    with pytest.raises(ValueError, match="3 alphas for 2 rows"):
        MS.post_filter(y, None, [0.8, 0.5, 0.1])
    with pytest.raises(ValueError, match="1 lens for 2 rows"):
        MS.post_filter(y, [5], 0.8)
    with pytest.raises(ValueError, match=r"wave must be float32 \[N, ld\] or \[ld\]"):
        MS.post_filter(y.double(), None, 0.8)


def _host_converter(post_filter):
    """the part of a converter the post filter's validation reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.post_filter = post_filter
    return c


def test_session_post_filter_is_checked_against_the_converter():
    assert "post_filter" in MS._PARAMS
    on, off = _host_converter(True), _host_converter(False)
    assert on._session_post_filter(0, dict(post_filter=0.7)) == 0.7 and on._session_post_filter(0, {}) == 0.0
    assert off._session_post_filter(1, dict(post_filter=0)) == 0.0 == off._session_post_filter(1, dict(post_filter=None))
    with pytest.raises(ValueError, match=r"slot 2: post_filter=0.5 needs a converter built with MultiStreamConverter\(..., post_filter=True\)"):
        off._session_post_filter(2, dict(post_filter=0.5))
    for bad in ("1", True, float("nan"), 0.9, -1):
        for conv in (on, off):
            with pytest.raises(ValueError, match=r"slot 1: post_filter=.* must be a finite number in \[0, 0.85\]"):
                conv._session_post_filter(1, dict(post_filter=bad))
    with pytest.raises(ValueError, match="post_filter must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, post_filter=0.8)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: post_filter_order=33 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, post_filter=True, post_filter_order=33)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: post_filter_ratio=2 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, post_filter=True, post_filter_ratio=2)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: post_filter_tilt=-1 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, post_filter=True, post_filter_tilt=-1)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: post_filter_window_ms=10 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, post_filter=True, post_filter_window_ms=10)
    with pytest.raises(ValueError, match=r"post_filter_db needs a converter built with MultiStreamConverter\(..., post_filter=True\)"):
        off.post_filter_db()
    assert MS.MultiStreamConverter.post_filter is False


def test_realtime_converter_checks_its_post_filter_before_anything_is_built():
    from module.realtime import RealtimeConverter
    for bad in ("0.5", True, 0.9, float("nan")):
        with pytest.raises(ValueError, match=r"post_filter=.* must be a finite number in \[0, 0.85\]"):
            RealtimeConverter(None, None, None, None, post_filter=bad)
    with pytest.raises(ValueError, match="post_filter_ratio='x' must be"):
        RealtimeConverter(None, None, None, None, post_filter=0.5, post_filter_ratio="x")
    with pytest.raises(ValueError, match="post_filter_order=0 must be"):
        RealtimeConverter(None, None, None, None, post_filter=0.5, post_filter_order=0)
    with pytest.raises(ValueError, match="post_filter_window_ms=70 must be"):
        RealtimeConverter(None, None, None, None, post_filter=0.5, post_filter_window_ms=70)
    assert RealtimeConverter.__new__(RealtimeConverter).post_filter is False


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_post_filter_symbol_is_exported_and_the_prototype_agrees_with_the_header():
    L = ctypes.CDLL(nat.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    name = "alive_postfilter_waves"
    assert hasattr(L, name)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert decl is not None, f"{name} is not declared in alive_vc.h"
    args = decl.group(1).split(",")
    assert len(args) == 18 == len(nat.PROTOTYPES[name][1]) and nat.PROTOTYPES[name][0] is ctypes.c_int
    kinds = [ctypes.c_void_p if "*" in a else (ctypes.c_double if "double" in a else ctypes.c_int) for a in args]
    assert kinds == nat.PROTOTYPES[name][1]
    mk = open(os.path.join(ROOT, "alive-vc_amd", "csrc", "Makefile")).read()
    assert "postfilter.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]
    assert "-ffp-contract=off" in mk and "-fno-fast-math" in mk and "-ffast-math" not in mk.replace("-fno-fast-math", "")


def test_post_filter_abi_refuses_bad_arguments():
    L = nat.lib()
    f = L.alive_postfilter_waves
    #     out   y      ld  N  len alpha hop  win  ord win lag ratio  tilt floor  g_lo  g_hi mm    stream
    ok = [4096, 16384, 64, 2, 16, 16,   320, 640, 16, 16, 16, 0.625, 0.5, 1e-10, 0.25, 4.0, None, None]
    for i in (0, 1, 5, 9, 10):
        a = list(ok)
        a[i] = None
        assert f(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((2, 0), (2, -1), (3, 0), (3, -1), (3, 65536)):
        a = list(ok)
        a[i] = bad
        assert f(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)
    for bad in (0, 1, 7, 321, 1026, -2):
        a = list(ok)
        a[6] = bad
        assert f(*a) == -1 and b"hop" in L.alive_last_error(), bad
    for bad in (1026, 2048, 641, 321, 318, 0, -640):                  # beyond 1024, an odd excess, under the hop
        a = list(ok)
        a[7] = bad
        assert f(*a) == -1 and b"window" in L.alive_last_error(), bad
    for bad in (0, -1, MS.POSTFILTER_MAX_ORDER + 1, 1000):
        a = list(ok)
        a[8] = bad
        assert f(*a) == -1 and b"order" in L.alive_last_error(), bad
    for i, word in ((11, b"ratio"), (12, b"tilt")):
        for bad in (float("nan"), float("inf"), float("-inf"), -0.5, 1.5):
            a = list(ok)
            a[i] = bad
            assert f(*a) == -1 and word in L.alive_last_error(), (i, bad)
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        a = list(ok)
        a[13] = bad
        assert f(*a) == -1 and b"floor" in L.alive_last_error(), bad
    for lo, hi in ((0.0, 4.0), (-0.5, 4.0), (1.5, 4.0), (0.25, 0.5), (float("nan"), 4.0), (0.25, float("inf")), (0.25, float("nan"))):
        a = list(ok)
        a[14], a[15] = lo, hi
        assert f(*a) == -1 and b"range" in L.alive_last_error(), (lo, hi)
    by = 2 * 64 * 4
    for out in (16384, 16384 + 4, 16384 - by + 4, 16384 + by - 4):
        a = list(ok)
        a[0] = out
        assert f(*a) == -1 and b"overlaps y" in L.alive_last_error(), out


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


def test_sessions_file_takes_a_post_filter_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    assert MSI.POSTFILTER_KEYS == ("post_filter",)
    a, b, c, d = MSI.load_sessions(write(files, [sess, dict(sess, post_filter=0.7), dict(sess, post_filter=0), dict(sess, post_filter=None)]))
    assert set(a) == set(MSI.SESSION_KEYS) == set(c) == set(d) and b["post_filter"] == 0.7
    assert set(b) == set(MSI.SESSION_KEYS) | {"post_filter"}
    # -pf is the default; a session's null or 0 switches it off, its own value wins
    a, b, c, d = MSI.load_sessions(write(files, [sess, dict(sess, post_filter=None), dict(sess, post_filter=0), dict(sess, post_filter=0.25)]),
                                   post_filter=0.5)
    assert a["post_filter"] == 0.5 and "post_filter" not in b and "post_filter" not in c and d["post_filter"] == 0.25
    for bad in ("0.5", True, [1], 0.9, -0.5):
        with pytest.raises(ValueError, match=r"session 1: post_filter="):
            MSI.load_sessions(write(files, [sess, dict(sess, post_filter=bad)]))
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['post_filter_ratio'\]"):
        MSI.load_sessions(write(files, [dict(sess, post_filter_ratio=0.5)]))
    with pytest.raises(ValueError, match=r"-pf / --post-filter-ratio / --post-filter-tilt: post_filter=3 must be"):
        MSI.load_sessions(write(files, [sess]), post_filter=3)
    with pytest.raises(ValueError, match=r"-pf / --post-filter-ratio / --post-filter-tilt: post_filter_tilt=7 must be"):
        MSI.load_sessions(write(files, [sess]), post_filter_tilt=7)


def test_jobs_file_takes_a_post_filter_per_job(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    assert BI.POSTFILTER_KEYS == ("post_filter",)
    a, b, c, d = BI.load_jobs(write(files, [job, dict(job, post_filter=0.7), dict(job, post_filter=0), dict(job, post_filter=None)]))
    assert set(a) == set(BI.JOB_KEYS) == set(c) == set(d) and b["post_filter"] == 0.7 and set(b) == set(BI.JOB_KEYS + BI.POSTFILTER_KEYS)
    a, b, c, d = BI.load_jobs(write(files, [job, dict(job, post_filter=None), dict(job, post_filter=0.0), dict(job, post_filter=0.85)]),
                              post_filter=0.5)
    assert a["post_filter"] == 0.5 and "post_filter" not in b and "post_filter" not in c and d["post_filter"] == 0.85
    for bad in ("1", True, 2, float("nan")):
        with pytest.raises(ValueError, match=r"job 1: post_filter="):
            BI.load_jobs(write(files, [job, dict(job, post_filter=bad)]))
    with pytest.raises(ValueError, match=r"job 0: unknown keys \['post_filter_tilt'\]"):
        BI.load_jobs(write(files, [dict(job, post_filter_tilt=0.5)]))
    with pytest.raises(ValueError, match=r"-pf / --post-filter-ratio / --post-filter-tilt: post_filter_ratio=-1 must be"):
        BI.load_jobs(write(files, [job]), post_filter_ratio=-1)


def test_all_four_clis_take_the_post_filter_flags():
    import inference as INF
    import realtime_inference as RI
    for mod, argv in ((INF, []), (RI, []), (BI, ["j.json"]), (MSI, ["s.json"])):
        args = mod.build_parser().parse_args(argv)
        assert (args.post_filter_alpha, args.post_filter_ratio, args.post_filter_tilt) == (0.0, 0.625, 0.5)
        assert isinstance(args.post_filter_alpha, float)
        args = mod.build_parser().parse_args(argv + ["-pf", "0.8", "--post-filter-ratio", "0.5", "--post-filter-tilt", "0.3"])
        assert (args.post_filter_alpha, args.post_filter_ratio, args.post_filter_tilt) == (0.8, 0.5, 0.3)
        assert mod.build_parser().parse_args(argv + ["--post-filter-alpha", "0.5"]).post_filter_alpha == 0.5
