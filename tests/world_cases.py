"""The cases of the WORLD pitch stage tests (tests/test_host_world_stages.py on the CPU, tests/test_gpu_world_stages.py on the device):
configurations, row lengths chosen by what they isolate in csrc/world_f0.hip, mixed rows, the plan of a call as a dict
(alive_world_f0_layout, host arithmetic) and the restatement's stage outputs (tools/world_ref.py dio_stages), computed once per case.

Every case is small: rows of at most 5000 samples, 3 or 4 rows per call.  A case whose StoneMask decisions come too close to a branch
(test_host_world_stages.py, stonemask_margin) gets another seed in RESEED, never an exclusion."""
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import world_ref as W   # noqa: E402

# (fs, f0_floor, f0_ceil, frame_period)
CONFIGS = [(8000, 20.0, 4096.0, 5.0),       # production: 16 bands down to h = 1
           (16000, 50.0, 800.0, 5.0),       # c = 320 (641 low-cut taps of the 801 the kernel holds), 9 bands
           (16000, 22.1, 4096.0, 5.0),      # h[0] = 256: the lowest band's 1024 taps fill the sweep's tile buffer exactly; 16 bands
           (8000, 20.0, 4096.0, 10.0)]      # voice range and frame count change
# One more, with one length and fixed rows: a frame period chosen so that the time of frame 25 IS the location of interval 13 of the
# negative-crossing stream of row 0, band 7, bit for bit -- and that interval is the newest one when the sweep leaves its first tile,
# its value more than twice its predecessor's.  This is the knot of interp1 (a location counts as passed when it is <= the frame's
# time) and the sweep's rule that a frame waits until an interval lies strictly past it: resolved a tile early, the frame would be
# extrapolated from the previous segment, which here rounds differently.  tests/test_host_world_stages.py checks all of this on
# the restatement.
GRID = len(CONFIGS)
KNOT = (8000, 20.0, 4096.0, 5.020788179536475)
KNOT_L, KNOT_KINDS, KNOT_AT = 2600, ("noise", "voice", "burst", "tone150"), dict(row=0, band=7, stream=0, interval=13, frame=25)
CONFIGS.append(KNOT)
# refused by plan(): a 1132-tap lowest band; a rate above 16 kHz; an empty range; a ceiling that rounds a band's half delay to 0
REFUSED = [(16000, 20.0, 4096.0, 5.0), (16001, 20.0, 4096.0, 5.0), (8000, 100.0, 100.0, 5.0), (8000, 100.0, 50.0, 5.0),
           (8000, 20.0, 20000.0, 5.0)]
MAX_L = 5000
LAYOUT_WORDS = 16 + 3 * 32
OFFSETS = ("mean", "yl", "iv", "ni", "best", "s1", "s2", "s3", "pos", "neg")     # ascending in the workspace, in stage order

KINDS = {8000: ("voice", "low", "high", "alt", "zeros", "burst", "noise", "glide_low", "glide_high", "tone150"),
         16000: ("voice", "low", "high", "alt", "zeros", "burst", "noise", "glide_low", "voice40", "tone150")}
# the lengths with a contour: rows that DIO finds voiced, so that select, FixF0Contour's steps 3-4 and StoneMask have work ("high":
# glide_high at 8 kHz, voice40 at 16 kHz)
CONTOUR = {2600: ("tone150", "voice", "high"), 3839: ("glide_low", "noise", "voice", "tone150"), 3840: ("voice", "low", "glide_low"),
           3841: ("high", "tone150", "burst", "voice"), 5000: ("glide_low", "high", "voice", "tone150")}
# (configuration index, L) -> seed bump, for the cases whose first seed left a StoneMask decision within 1e-5 of a branch
RESEED = {(0, 3840): 1, (1, 3839): 1, (1, 3841): 1, (2, 5000): 1, (3, 3072): 1, (3, 3839): 1, (3, 3841): 2}


def _first_L(fs, period, frames):
    """the smallest L with n_frames(L) == frames"""
    L = 1
    while W.n_frames(L, fs, period) < frames:
        L += 1
    assert W.n_frames(L, fs, period) == frames
    return L


def lengths(cfg):
    fs, lo, _, period = cfg
    if cfg == KNOT:
        return [KNOT_L]
    c = W.matlab_round(fs / W.K_CUTOFF)
    vr = W.voice_range(period, lo)
    seam = 8 * 256 - 1 - 2 * c                                  # yl_ld = L + 1 + 2c = 2048: the low cut's last block is full
    out = [1, 2, 3,                                             # F = 1; the sweep's pp >= 1 and pp >= 2
           100, 800, _first_L(fs, period, vr), _first_L(fs, period, vr + 1),      # F below, at and one past the voice range
           1022, 1023, 1024, 1025,                              # Ly = L + 1 straddles one sweep tile
           2047, 2048, 2049, 3071, 3072,                        # the second and third seam
           seam - 1, seam, seam + 1,                            # yl_ld = 255, 0, 1 mod 256
           2600, 3839, 3840, 3841, 5000]                        # a contour that FixF0Contour's edges do not blank
    assert max(out) <= MAX_L
    return sorted(set(out))


def cases():
    """(configuration index, L) of every case"""
    return [(ci, L) for ci, cfg in enumerate(CONFIGS) for L in lengths(cfg)]


def case_id(case):
    fs, lo, hi, period = CONFIGS[case[0]]
    return f"{fs}-{lo:g}-{hi:g}-{period:g}ms-L{case[1]}"


def case_kinds(case):
    ci, L = case
    cfg = CONFIGS[ci]
    i = lengths(cfg).index(L)
    kinds = KINDS[cfg[0]]
    if cfg == KNOT:
        return list(KNOT_KINDS)
    if L in CONTOUR:
        return [("glide_high" if cfg[0] == 8000 else "voice40") if k == "high" else k for k in CONTOUR[L]]
    return [kinds[(3 * i + j) % len(kinds)] for j in range(3 + i % 2)]


def _glide(rs, t, fs, a, b, harmonics):
    f = a + (b - a) * t / max(t[-1], 1.0 / fs)
    ph = 2 * np.pi * np.cumsum(f) / fs
    return sum(0.3 / k * np.sin(k * ph + rs.uniform(0, 6.28)) for k in range(1, harmonics + 1))


def make_row(kind, L, fs, rs):
    t = np.arange(L) / float(fs)
    if kind == "voice":                                         # a harmonic voice with vibrato
        f0 = rs.uniform(70, 400)
        f = f0 * (1 + 0.04 * np.sin(2 * np.pi * rs.uniform(3, 7) * t))
        ph = 2 * np.pi * np.cumsum(f) / fs
        return sum(0.3 / k * np.sin(k * ph + rs.uniform(0, 6.28)) for k in range(1, 9))
    if kind == "low":                                           # two or three events per tile; 0 .. 3 intervals at short L
        return 0.5 * np.sin(2 * np.pi * rs.uniform(25, 30) * t + rs.uniform(0, 6.28))
    if kind == "high":                                          # an event every other sample in the top bands
        return 0.4 * np.sin(2 * np.pi * 3500.0 * t + rs.uniform(0, 6.28))
    if kind == "alt":
        return rs.uniform(0.2, 0.9) * (1.0 - 2.0 * (np.arange(L) % 2))
    if kind == "zeros":
        return np.zeros(L)
    if kind == "burst":                                         # tiles without events after a tile with some
        x = np.zeros(L)
        at = rs.randint(0, max(1, min(L, 1000) - 20))
        n = min(20, L - at)
        x[at:at + n] = 0.5 * rs.randn(n)
        return x
    if kind == "noise":
        return 0.1 * rs.randn(L)
    if kind == "glide_low":                                     # across StoneMask's 40-Hz gate
        return _glide(rs, t, fs, 38.0, 45.0, 4)
    if kind == "glide_high":                                    # across StoneMask's fs / 12 gate at 8 kHz
        return _glide(rs, t, fs, 640.0, 690.0, 4)
    if kind == "voice40":                                       # StoneMask windows of up to 1201 samples at 16 kHz
        return _glide(rs, t, fs, 40.5, 42.0, 6)
    if kind == "tone150":
        return sum(0.3 / k * np.sin(2 * np.pi * k * 150.0 * t + rs.uniform(0, 6.28)) for k in range(1, 7))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case_rows(case):
    """float32 [N, L], read only"""
    ci, L = case
    rs = np.random.RandomState(10007 * ci + L + 100000 * RESEED.get(case, 0))
    X = np.stack([make_row(k, L, CONFIGS[ci][0], rs) for k in case_kinds(case)]).astype(np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=4)
def case_stages(case):
    """(dio_stages rows, t) of the case: the one reference of every stage test, left unchanged"""
    return W.dio_stages(case_rows(case).astype(np.float64), *CONFIGS[case[0]])


def layout(lib, N, L, cfg):
    """alive_world_f0_layout as a dict (offsets in bytes under the names of OFFSETS), or its negative code"""
    out = (ctypes.c_int64 * LAYOUT_WORDS)()
    n = lib.alive_world_f0_layout(N, L, cfg[0], cfg[1], cfg[2], cfg[3], ctypes.cast(out, ctypes.c_void_p), LAYOUT_WORDS)
    if n < 0:
        return n
    o = list(out)[:n]
    v = dict(zip(("F", "nb", "c", "Ly", "yl_ld", "total"), o[:6]))
    v["off"] = dict(zip(OFFSETS, o[6:16]))
    nb = v["nb"]
    assert n == 16 + 3 * nb
    v["h"], v["woff"] = o[16:16 + nb], o[16 + nb:16 + 2 * nb]
    v["bound"] = np.array(o[16 + 2 * nb:16 + 3 * nb], dtype=np.int64).view(np.float64)
    return v
