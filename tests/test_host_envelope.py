"""CPU tests of the envelope follow: the NumPy restatement tools/envelope_ref.py (identity at amount 0, silence, a silent source, y = x / 2
brought back to x within a derived bound, non-finite samples, the shortest rows, a row alone and stacked, level tracking on a modulated
source), check_envelope with every refusal, the validation on converters without a device, the sessions and jobs files, the flags of all
four CLIs, and the C ABI (symbol, prototype, refusals)."""
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
import envelope_ref as ER                                            # noqa: E402
import batch_inference as BI                                         # noqa: E402
import multistream_inference as MSI                                  # noqa: E402

HOP = 320


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def _noise(n, seed, scale=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_constants_are_those_of_the_python_wrapper():
    assert (ER.TILE, ER.MAX_RADIUS, ER.HOP) == (MS.ENVELOPE_TILE, MS.ENVELOPE_MAX_RADIUS, MS.ENVELOPE_HOP)
    assert ER.constants() == MS.check_envelope(1.0)[1:4] == (1e-6, 10.0 ** -0.6, 10.0 ** 0.6)
    assert ER.constants(-47.5, 7.25) == MS.check_envelope(0.3, -47.5, 7.25, 3)[1:4]
    hdr = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    assert f"#define ALIVE_ENVELOPE_TILE {ER.TILE}\n" in hdr and f"#define ALIVE_ENVELOPE_MAX_RADIUS {ER.MAX_RADIUS}\n" in hdr


def test_frame_sums_follow_the_stated_order():
    """the order, written out element by element for one frame of 320 + a short last frame"""
    v = _noise(HOP + 77, 1, 0.5)
    S = ER.frame_sums(v, len(v), HOP)
    assert S.shape == (2,) and S.dtype == np.float64
    for f, cnt in ((0, HOP), (1, 77)):
        acc = [0.0] * 256
        for j in range(2):
            for a in range(256):
                e = a + 256 * j
                if e < cnt:
                    acc[a] = acc[a] + float(v[f * HOP + e]) * float(v[f * HOP + e])
        s = [(acc[4 * l] + acc[4 * l + 1]) + (acc[4 * l + 2] + acc[4 * l + 3]) for l in range(64)]
        o = 32
        while o:
            for l in range(o):
                s[l] = s[l] + s[l + o]
            o >>= 1
        assert S[f] == s[0]
    assert abs(S[0] - np.sum(v[:HOP].astype(np.float64) ** 2)) <= 1e-13 * S[0]


def test_amount_zero_is_the_identity_bitwise():
    y, x = _noise((2, 2000), 2), _noise((2, 2000), 3, 0.4)
    y[0, 5], y[0, 6], y[1, 7], y[1, 8] = -0.0, 0.0, np.nan, np.inf
    out, G, mm = ER.envelope_waves(y, x, None, 0.0)
    assert np.array_equal(_bits(out), _bits(y)) and G == [None, None] and mm.tolist() == [[1.0, 1.0]] * 2
    for bad in (1.5, float("nan"), -0.25):                           # an amount outside (0, 1]: copied
        assert np.array_equal(_bits(ER.envelope_waves(y, x, None, bad)[0]), _bits(y))
    out, G, _ = ER.envelope_waves(y, x, [0, -3], 1.0)                # no samples: copied
    assert np.array_equal(_bits(out), _bits(y)) and G == [None, None]
    out, G, _ = ER.envelope_waves(y[:1], x[:1], [700], 1.0)          # samples at or beyond n: copied
    assert np.array_equal(_bits(out[0, 700:]), _bits(y[0, 700:])) and not np.array_equal(out[0, :700], y[0, :700]) and len(G[0]) == 3


def test_silence_and_a_silent_source():
    z = np.zeros((1, 5 * HOP + 9), np.float32)
    out, G, mm = ER.envelope_waves(z, z, None, 1.0)
    assert np.all(G[0] == 1.0) and not out.any() and mm.tolist() == [[1.0, 1.0]]
    y = _noise((1, 5 * HOP + 9), 4, 0.5)
    out, G, mm = ER.envelope_waves(y, z, None, 1.0)
    g_lo = ER.constants()[1]
    assert np.all(G[0] == g_lo) and mm[0, 0] == mm[0, 1] == np.float32(g_lo)
    assert np.array_equal(out[0], (y[0].astype(np.float64) * g_lo).astype(np.float32))
    out, G, _ = ER.envelope_waves(y, z, None, 0.25)                  # the blend is linear in gain
    assert np.all(G[0] == 1.0 + 0.25 * (g_lo - 1.0))
    out, G, _ = ER.envelope_waves(z + np.float32(1e-5), y, None, 1.0)     # a loud source against a faint output: the other end
    assert np.all(G[0] == ER.constants()[2])


def test_half_the_source_comes_back_as_the_source():
    """y = x / 2 is exact in float32.  With floor_db = -200 (e = 1e-20) and every frame's mean square M >= 1e-8, e / M <= 1e-12, so
    q = 4 (1 + O(1e-12)) and sqrt(q) = 2 (1 + O(1e-12)); the fp64 roundings add about 1e-15 and the one float32 rounding of the
    product 6e-8: |out - x| <= 1e-6 |x| with room to spare"""
    rng = np.random.default_rng(5)
    n = 23 * HOP + 141
    t = np.arange(n)
    x = ((0.02 + 0.5 * (1 + np.sin(2 * np.pi * t / 4000.0))) * rng.standard_normal(n)).astype(np.float32)
    y = (x * np.float32(0.5)).astype(np.float32)
    assert np.array_equal(y.astype(np.float64) * 2, x.astype(np.float64))
    assert (ER.frame_sums(x, n, HOP) / np.r_[[HOP] * 23, [141]]).min() >= 1e-8
    for R in (0, 1, 4):
        out = ER.follow(y, x, 1.0, floor_db=-200.0, radius=R)
        assert np.all(np.abs(out.astype(np.float64) - x) <= 1e-6 * np.abs(x)), R
    half = ER.follow(y, x, 0.5, floor_db=-200.0)                      # half way in gain: 1.5 y = 0.75 x
    assert np.all(np.abs(half.astype(np.float64) - 0.75 * x) <= 1e-6 * np.abs(x))


@pytest.mark.parametrize("R", [0, 1, 2, 4])
def test_non_finite_samples_leave_exactly_the_frames_within_R_at_unity(R):
    n = 30 * HOP
    x, y = _noise(n, 6, 0.4), _noise(n, 7, 0.05)
    y[8 * HOP + 3] = np.nan
    x[20 * HOP - 1] = np.inf                                         # the last sample of frame 19
    e, g_lo, g_hi = ER.constants()
    G = ER.frame_gains(x, y, n, 1.0, HOP, R, e, g_lo, g_hi)
    clean_x, clean_y = x.copy(), y.copy()
    clean_y[8 * HOP + 3], clean_x[20 * HOP - 1] = 0.0, 0.0
    G0 = ER.frame_gains(clean_x, clean_y, n, 1.0, HOP, R, e, g_lo, g_hi)
    touched = np.zeros(30, bool)
    touched[8 - R:8 + R + 1] = True
    touched[19 - R:19 + R + 1] = True
    assert np.all(G[touched] == 1.0) and np.all(G0[touched] != 1.0)
    assert np.array_equal(G[~touched], G0[~touched])                 # no other frame changes
    out = ER.follow(y, x, 1.0, radius=R)
    assert np.isnan(out[8 * HOP + 3]) and np.isfinite(np.delete(out, 8 * HOP + 3)).all()


def test_the_shortest_rows():
    for n, F in ((1, 1), (HOP - 1, 1), (HOP, 1), (HOP + 1, 2), (2 * HOP + 1, 3)):
        x, y = _noise(n, 8 + n, 0.3), _noise(n, 9 + n, 0.1)
        out, G, mm = ER.envelope_waves(y[None], x[None], None, 1.0)
        assert G[0].shape == (F,) and np.isfinite(out).all() and out.shape == (1, n) and np.isfinite(G[0]).all()
        assert mm[0, 0] == np.float32(G[0].min()) and mm[0, 1] == np.float32(G[0].max())
        g = ER.sample_gains(G[0], n, HOP)
        assert g[0] == G[0][0]
        if F == 1 or n - 1 >= HOP // 2 + (F - 1) * HOP:                       # (a last frame shorter than half a hop never reaches its centre)
            assert g[-1] == G[0][-1]
        else:
            assert F > 1 and min(G[0][-2:]) <= g[-1] <= max(G[0][-2:])
        if F == 1:
            assert np.all(g == G[0][0])
    # the interpolation: constant over the first and the last half frame, the frame's own gain at its centre, linear between
    G = np.array([1.0, 2.0, 0.5])
    g = ER.sample_gains(G, 3 * HOP, HOP)
    c = HOP // 2
    assert np.all(g[:c + 1] == 1.0) and g[c + HOP] == 2.0 and np.all(g[c + 2 * HOP:] == 0.5)
    assert g[c + HOP // 4] == 1.0 + (2.0 - 1.0) * 0.25 and g[c + HOP + HOP // 2] == 2.0 + (0.5 - 2.0) * 0.5


def test_a_row_is_the_same_alone_and_stacked():
    n = 9 * HOP + 17
    ys, xs = _noise((4, n), 10, 0.2), _noise((4, n + 5), 11, 0.3)    # (x rows longer than y rows)
    lens, amounts = [n, 5 * HOP, n - 1, 3], [1.0, 0.5, 0.0, 0.75]
    out, G, mm = ER.envelope_waves(ys, xs, lens, amounts, radius=2)
    for r in range(4):
        o1, G1, m1 = ER.envelope_waves(ys[r:r + 1], xs[r:r + 1], lens[r:r + 1], amounts[r], radius=2)
        assert np.array_equal(_bits(o1[0]), _bits(out[r])) and np.array_equal(m1[0], mm[r])
        assert (G1[0] is None and G[r] is None) or np.array_equal(G1[0], G[r])
    # hop 8: the same function at another frame size
    o8 = ER.envelope_waves(ys, xs, lens, amounts, hop=8, radius=2)[0]
    assert not np.array_equal(o8[0], out[0]) and np.array_equal(_bits(o8[2]), _bits(ys[2]))


def test_the_converted_level_tracks_a_modulated_source():
    """white noise against an amplitude-modulated source: the per-frame level follows it"""
    rng = np.random.default_rng(12)
    n = 200 * HOP
    t = np.arange(n)
    x = ((0.05 + 0.25 * (1 + np.sin(2 * np.pi * t / 16000.0))) * rng.standard_normal(n)).astype(np.float32)
    y = (0.2 * rng.standard_normal(n)).astype(np.float32)
    out = ER.follow(y, x, 1.0)

    def level(v):
        return 10 * np.log10(np.mean(v.astype(np.float64).reshape(-1, HOP) ** 2, axis=1))
    before, after = np.corrcoef(level(y), level(x))[0, 1], np.corrcoef(level(out), level(x))[0, 1]
    err = np.median(np.abs(level(out) - level(x)))
    print(f"frame level correlation {before:.2f} -> {after:.2f}, median frame level error {err:.2f} dB")
    assert abs(before) < 0.2 and after > 0.9 and err < 1.0


# ------------------------------------------------------------------------------------------------ the settings
def test_check_envelope():
    assert MS.check_envelope(0) == (0.0, 1e-6, 10.0 ** -0.6, 10.0 ** 0.6, 1)
    assert MS.check_envelope(1, -40, 0, 0) == (1.0, 1e-4, 1.0, 1.0, 0)
    assert MS.check_envelope(np.float32(0.5), -60, 6, np.int64(4))[::4] == (0.5, 4)
    for bad in (-0.1, 1.01, float("nan"), float("inf"), "0.5", True, None, [0.5]):
        with pytest.raises(ValueError, match=r"envelope=.* must be a finite number in \[0, 1\]"):
            MS.check_envelope(bad)
    for bad in (float("nan"), float("-inf"), "x", True, None, -4000, 4000):
        with pytest.raises(ValueError, match="envelope_floor_db=.* must be"):
            MS.check_envelope(0.5, bad)
    for bad in (-1, float("nan"), float("inf"), "6", False, None, 7000):
        with pytest.raises(ValueError, match="envelope_range_db=.* must be"):
            MS.check_envelope(0.5, -60, bad)
    for bad in (-1, 5, 1.0, True, None, "1"):
        with pytest.raises(ValueError, match=r"envelope_radius=.* must be an integer in \[0, 4\]"):
            MS.check_envelope(0.5, -60, 12, bad)
    assert MS.minmax_db([(1.0, 1.0), (0.5, 2.0)]) == [(0.0, 0.0), (20 * np.log10(0.5), 20 * np.log10(2.0))]


def _host_converter(envelope):
    """the part of a converter the envelope's validation reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.envelope = envelope
    return c


def test_session_envelope_is_checked_against_the_converter():
    assert "envelope" in MS._PARAMS
    on, off = _host_converter(True), _host_converter(False)
    assert on._session_envelope(0, dict(envelope=0.7)) == 0.7 and on._session_envelope(0, {}) == 0.0
    assert off._session_envelope(1, dict(envelope=0)) == 0.0 == off._session_envelope(1, dict(envelope=None))
    with pytest.raises(ValueError, match=r"slot 2: envelope=0.5 needs a converter built with MultiStreamConverter\(..., envelope=True\)"):
        off._session_envelope(2, dict(envelope=0.5))
    for bad in ("1", True, float("nan"), 2, -1):
        for conv in (on, off):
            with pytest.raises(ValueError, match=r"slot 1: envelope=.* must be a finite number in \[0, 1\]"):
                conv._session_envelope(1, dict(envelope=bad))
    with pytest.raises(ValueError, match="envelope must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, envelope=1)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: envelope_radius=5 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, envelope=True, envelope_radius=5)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: envelope_range_db=-1 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, envelope=True, envelope_range_db=-1)
    with pytest.raises(ValueError, match=r"envelope_db needs a converter built with MultiStreamConverter\(..., envelope=True\)"):
        off.envelope_db()
    assert MS.MultiStreamConverter.envelope is False


def test_realtime_converter_checks_its_envelope_before_anything_is_built():
    from module.realtime import RealtimeConverter
    for bad in ("0.5", True, 2, float("nan")):
        with pytest.raises(ValueError, match=r"envelope=.* must be a finite number in \[0, 1\]"):
            RealtimeConverter(None, None, None, None, envelope=bad)
    with pytest.raises(ValueError, match="envelope_floor_db='x' must be"):
        RealtimeConverter(None, None, None, None, envelope=0.5, envelope_floor_db="x")
    with pytest.raises(ValueError, match="envelope_radius=9 must be"):
        RealtimeConverter(None, None, None, None, envelope=0.5, envelope_radius=9)
    assert RealtimeConverter.__new__(RealtimeConverter).envelope is False


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_envelope_symbol_is_exported_and_the_prototype_agrees_with_the_header():
    L = ctypes.CDLL(nat.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    name = "alive_envelope_waves"
    assert hasattr(L, name)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert decl is not None, f"{name} is not declared in alive_vc.h"
    args = decl.group(1).split(",")
    assert len(args) == 15 == len(nat.PROTOTYPES[name][1]) and nat.PROTOTYPES[name][0] is ctypes.c_int
    kinds = [ctypes.c_void_p if "*" in a else (ctypes.c_double if "double" in a else ctypes.c_int) for a in args]
    assert kinds == nat.PROTOTYPES[name][1]
    mk = open(os.path.join(ROOT, "alive-vc_amd", "csrc", "Makefile")).read()
    assert "envelope.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]
    assert "-ffp-contract=off" in mk and "-fno-fast-math" in mk and "-ffast-math" not in mk.replace("-fno-fast-math", "")


def test_envelope_abi_refuses_bad_arguments():
    L = nat.lib()
    #     out   y      ld_y x      ld_x N  len amount hop  R  floor g_lo g_hi mm    stream
    ok = [4096, 16384, 64,  32768, 80,  2, 16, 16,    320, 1, 1e-6, 0.25, 4.0, None, None]
    for i in (0, 1, 3, 7):
        a = list(ok)
        a[i] = None
        assert L.alive_envelope_waves(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((2, 0), (2, -1), (4, 0), (4, -3), (5, 0), (5, -1), (5, 65536)):
        a = list(ok)
        a[i] = bad
        assert L.alive_envelope_waves(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)
    for bad in (0, 1, 7, 321, 1026, -2):
        a = list(ok)
        a[8] = bad
        assert L.alive_envelope_waves(*a) == -1 and b"hop" in L.alive_last_error(), bad
    for bad in (-1, MS.ENVELOPE_MAX_RADIUS + 1):
        a = list(ok)
        a[9] = bad
        assert L.alive_envelope_waves(*a) == -1 and b"radius" in L.alive_last_error(), bad
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        a = list(ok)
        a[10] = bad
        assert L.alive_envelope_waves(*a) == -1 and b"floor" in L.alive_last_error(), bad
    for lo, hi in ((0.0, 4.0), (-0.5, 4.0), (1.5, 4.0), (0.25, 0.5), (float("nan"), 4.0), (0.25, float("inf")), (0.25, float("nan"))):
        a = list(ok)
        a[11], a[12] = lo, hi
        assert L.alive_envelope_waves(*a) == -1 and b"range" in L.alive_last_error(), (lo, hi)
    by, bx = 2 * 64 * 4, 2 * 80 * 4
    for out, msg in ((16384, b"overlaps y"), (16384 + 4, b"overlaps y"), (16384 - by + 4, b"overlaps y"), (16384 + by - 4, b"overlaps y"),
                     (32768, b"overlaps x"), (32768 + bx - 4, b"overlaps x"), (32768 - by + 4, b"overlaps x")):
        a = list(ok)
        a[0] = out
        assert L.alive_envelope_waves(*a) == -1 and msg in L.alive_last_error(), out


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


def test_sessions_file_takes_an_envelope_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    assert MSI.ENVELOPE_KEYS == ("envelope",)
    a, b, c, d = MSI.load_sessions(write(files, [sess, dict(sess, envelope=0.7), dict(sess, envelope=0), dict(sess, envelope=None)]))
    assert set(a) == set(MSI.SESSION_KEYS) == set(c) == set(d) and b["envelope"] == 0.7 and set(b) == set(MSI.SESSION_KEYS) | {"envelope"}
    assert isinstance(MSI.load_sessions(write(files, [dict(sess, envelope=1)]))[0]["envelope"], float)
    # -env is the default; a session's null or 0 switches it off, its own value wins
    a, b, c, d = MSI.load_sessions(write(files, [sess, dict(sess, envelope=None), dict(sess, envelope=0), dict(sess, envelope=0.25)]),
                                   envelope=0.5)
    assert a["envelope"] == 0.5 and "envelope" not in b and "envelope" not in c and d["envelope"] == 0.25
    for bad in ("0.5", True, [1], 2, -0.5):
        with pytest.raises(ValueError, match=r"session 1: envelope="):
            MSI.load_sessions(write(files, [sess, dict(sess, envelope=bad)]))
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['envelope_radius'\]"):
        MSI.load_sessions(write(files, [dict(sess, envelope_radius=2)]))
    with pytest.raises(ValueError, match=r"-env / --envelope-floor / --envelope-range / --envelope-radius: envelope=3 must be"):
        MSI.load_sessions(write(files, [sess]), envelope=3)
    with pytest.raises(ValueError, match=r"-env / --envelope-floor / --envelope-range / --envelope-radius: envelope_radius=7 must be"):
        MSI.load_sessions(write(files, [sess]), envelope_radius=7)
    with pytest.raises(ValueError, match=r"envelope_range_db=-2 must be"):
        MSI.load_sessions(write(files, [sess]), envelope_range_db=-2)


def test_jobs_file_takes_an_envelope_per_job(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    assert BI.ENVELOPE_KEYS == ("envelope",)
    a, b, c, d = BI.load_jobs(write(files, [job, dict(job, envelope=0.7), dict(job, envelope=0), dict(job, envelope=None)]))
    assert set(a) == set(BI.JOB_KEYS) == set(c) == set(d) and b["envelope"] == 0.7 and set(b) == set(BI.JOB_KEYS + BI.ENVELOPE_KEYS)
    a, b, c, d = BI.load_jobs(write(files, [job, dict(job, envelope=None), dict(job, envelope=0.0), dict(job, envelope=1)]), envelope=0.5)
    assert a["envelope"] == 0.5 and "envelope" not in b and "envelope" not in c and d["envelope"] == 1.0
    for bad in ("1", True, 2, float("nan")):
        with pytest.raises(ValueError, match=r"job 1: envelope="):
            BI.load_jobs(write(files, [job, dict(job, envelope=bad)]))
    with pytest.raises(ValueError, match=r"job 0: unknown keys \['envelope_floor'\]"):
        BI.load_jobs(write(files, [dict(job, envelope_floor=-50)]))
    with pytest.raises(ValueError, match=r"-env / --envelope-floor / --envelope-range / --envelope-radius: envelope_floor_db=-4000 must be"):
        BI.load_jobs(write(files, [job]), envelope_floor_db=-4000)


def test_all_four_clis_take_the_envelope_flags():
    import inference as INF
    import realtime_inference as RI
    for mod, argv in ((INF, []), (RI, []), (BI, ["j.json"]), (MSI, ["s.json"])):
        args = mod.build_parser().parse_args(argv)
        assert (args.envelope, args.envelope_floor, args.envelope_range, args.envelope_radius) == (0.0, -60.0, 12.0, 1)
        assert isinstance(args.envelope_radius, int)
        args = mod.build_parser().parse_args(argv + ["-env", "0.7", "--envelope-floor", "-50", "--envelope-range", "6", "--envelope-radius",
                                                     "2"])
        assert (args.envelope, args.envelope_floor, args.envelope_range, args.envelope_radius) == (0.7, -50.0, 6.0, 2)
        assert mod.build_parser().parse_args(argv + ["--envelope", "1"]).envelope == 1.0
