"""CPU tests of pitch range: the four new entry points' symbols, prototypes and refusals; the NumPy restatement
(tools/pitch_range_ref.py) against a direct float64 mean / variance and on hand-made cases; a voice's range on the pool's host side
(3-tuple registers, merge on extend, set_register(range_st=), blend_range); the converters' argument checks; and the sessions / jobs
files ("intonation", "auto_range", "range_st"; a file without the keys parses to what it did)."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from module import _native as nat
from module import multistream as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "alive-vc_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import batch_inference as BI                                         # noqa: E402
import multistream_inference as MSI                                  # noqa: E402
import pitch_range_ref as RR                                         # noqa: E402
import pitch_ref as PR                                               # noqa: E402

NEW = ("alive_pitch_stats2_groups", "alive_pitch_range_groups", "alive_pitch_follow2_rows", "alive_pitch_transform_rows_centred")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_the_prototypes_agree_with_the_header():
    L = nat.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl is not None, f"{name} is not declared in alive_vc.h"
        args = decl.group(1).split(",")
        kinds = [ctypes.c_void_p if "*" in a else (ctypes.c_double if "double" in a else ctypes.c_int) for a in args]
        assert nat.PROTOTYPES[name][0] is ctypes.c_int and kinds == nat.PROTOTYPES[name][1], name
    mk = open(os.path.join(ROOT, "alive-vc_amd", "csrc", "Makefile")).read()
    assert "-ffp-contract=off" in mk and "pitch_auto.hip" in mk


def test_the_abi_refuses_bad_arguments():
    L = nat.lib()
    # stats2: as alive_pitch_stats_groups
    assert L.alive_pitch_stats2_groups(None, 1, 1, 0, 1, 16, 1, 16, None) == -1 and b"null" in L.alive_last_error()
    assert L.alive_pitch_stats2_groups(16, 1, 1, 0, 1, 16, 1, None, None) == -1 and b"null" in L.alive_last_error()
    for n, t, g in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert L.alive_pitch_stats2_groups(16, n, t, 0, 0, 16, g, 16, None) == -1
    for lo, hi in ((-1, 4), (3, 2), (0, 9)):
        assert L.alive_pitch_stats2_groups(16, 2, 8, lo, hi, 16, 1, 16, None) == -1 and b"outside [0, 8)" in L.alive_last_error()
    # range_groups: (stats3, first, G, N, inton, range_on, target_sd, range_max, inton_out, centre_out, centre_on_out, stream)
    ok = [16, 16, 1, 1, 16, 16, 16, 2.0, 16, 16, 16, None]
    for i in (0, 1, 4, 5, 6, 8, 9, 10):
        a = list(ok)
        a[i] = None
        assert L.alive_pitch_range_groups(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((2, 0), (3, 0), (7, 0.5), (7, float("inf")), (7, float("nan"))):
        a = list(ok)
        a[i] = bad
        assert L.alive_pitch_range_groups(*a) == -1, (i, bad)
    assert b"range_max" in L.alive_last_error()
    # follow2: (f0, N, T, f0_rate, offset, auto_on, target, inton, range_on, target_sd, emit, decay, prior, range_max, state3,
    #           shift_out, inton_out, centre_out, centre_on_out, stream)
    ok = [16, 2, 8, 16, 16, 16, 16, 16, 16, 16, 16, 0.5, 1.0, 2.0, 16, 16, 16, 16, 16, None]
    for i in (0, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15, 16, 17, 18):
        a = list(ok)
        a[i] = None
        assert L.alive_pitch_follow2_rows(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((1, 0), (2, 0), (11, -0.1), (11, 1.5), (11, float("nan")), (12, -1.0), (13, 0.99), (13, float("inf")),
                   (13, float("nan"))):
        a = list(ok)
        a[i] = bad
        assert L.alive_pitch_follow2_rows(*a) == -1, (i, bad)
    # centred transform: (f0, N, T, mode, f0_rate, shift, inton, centre, centre_on, stream)
    ok = [16, 2, 8, 1, 16, 16, 16, 16, 16, None]
    for i in (0, 4, 5, 6, 7, 8):
        a = list(ok)
        a[i] = None
        assert L.alive_pitch_transform_rows_centred(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((1, 0), (2, 0), (3, 2), (3, -1)):
        a = list(ok)
        a[i] = bad
        assert L.alive_pitch_transform_rows_centred(*a) == -1, (i, bad)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restated_sums_against_a_direct_float64_mean_and_variance():
    """Random pitch with |mean| <= 64 and sd >= 0.5.  The kernels' order differs from NumPy's pairwise sums by a few ulps of the sums;
    the variance Q / W - m^2 cancels at most (64^2 + sd^2) / sd^2 <= 2^14 + 1 of them: about 2^14 ulps, 4e-12 relative -- the bar is
    1e-10."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for mean, sd, T in ((-64.0, 0.5, 300), (-20.0, 0.5, 1), (0.0, 3.0, 255), (31.0, 1.0, 257), (64.0, 0.5, 2000), (-9.0, 12.0, 777)):
        N = 3
        p = rng.normal(mean, sd, size=(N, T))
        f0 = (440.0 * 2.0 ** ((p + 9.0) / 12.0)).astype(np.float32)
        f0[:, ::7] = 0.0 if T > 7 else f0[:, ::7]
        st = RR.stats2_groups(f0, [0, 1, N])
        for g, rows in enumerate((f0[:1], f0[1:])):
            pp = PR.pitch(rows)
            pv = pp[PR.voiced(pp)].astype(np.float64)
            assert st[g, 1] == pv.size > 0
            assert abs(st[g, 0] - pv.sum()) <= 1e-10 * np.abs(pv).sum()
            assert abs(st[g, 2] - (pv * pv).sum()) <= 1e-10 * (pv * pv).sum()
            if pv.size > 1:
                m, v = RR.mean_var(*st[g])
                assert abs(m - pv.mean()) <= 1e-10 * max(1.0, abs(pv.mean()))
                err = abs(v - pv.var()) / pv.var()
                worst = max(worst, err)
                assert err <= 1e-10, (mean, sd, T, err)
    print(f"worst relative variance error {worst:.2e}")
    # the first two columns are the two-moment restatement's, to the reordering of the sum
    f0 = rng.uniform(30.0, 4000.0, size=(4, 300)).astype(np.float32)
    a, b = RR.stats2_groups(f0, [0, 2, 2, 4], 7, 290), PR.stats_groups(f0, [0, 2, 2, 4], 7, 290)
    assert np.array_equal(a[:, 1], b[:, 1]) and np.allclose(a[:, 0], b[:, 0], rtol=1e-12, atol=0) and a[1].tolist() == [0.0] * 3


def test_restated_row_sums_follow_the_stated_order():
    """the order written out element by element: thread tid takes frames tid, tid + 256, ..., then the tree"""
    rng = np.random.default_rng(2)
    f0 = rng.uniform(50.0, 900.0, size=600).astype(np.float32)
    f0[::9] = 0.0
    p = PR.pitch(f0)
    s, q = [0.0] * 256, [0.0] * 256
    for tid in range(256):
        for t in range(tid, 600, 256):
            if np.isfinite(p[t]):
                s[tid] += float(p[t])
                q[tid] += float(p[t]) * float(p[t])
    o = 128
    while o:
        for tid in range(o):
            s[tid] += s[tid + o]
            q[tid] += q[tid + o]
        o //= 2
    assert RR.row_sums(f0) == (s[0], int(np.isfinite(p).sum()), q[0])


def test_restated_range_factor_and_groups():
    assert RR.range_factor(4.0, 3.0, 2.0) == 1.5 and RR.range_factor(4.0, 8.0, 2.0) == 2.0 and RR.range_factor(4.0, 0.5, 2.0) == 0.5
    for v, sd in ((0.0, 1.0), (-1e-9, 1.0), (1.0, 0.0), (1.0, -2.0), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0),
                  (1.0, float("inf"))):
        assert RR.range_factor(v, sd, 2.0) == 1.0, (v, sd)
    assert RR.range_factor(4.0, 100.0, 1.0) == 1.0                     # range_max 1: auto range can do nothing
    # groups: sums (s, c, q) with mean -10 and variance 4 / mean 3 and variance 0 / nothing voiced / off
    stats = np.array([[-40.0, 4.0, 416.0], [6.0, 2.0, 18.0], [0.0, 0.0, 0.0], [-40.0, 4.0, 416.0]])
    first = [0, 2, 3, 3, 5]
    it, c, on = RR.range_groups(stats, first, [1.5, 0.7, 1.0, 1.25], [1, 1, 1, 0], [3.0, 5.0, 1.0, 3.0], 2.0)
    assert it.dtype == c.dtype == np.float32 and on.dtype == np.int32
    assert it.tolist() == [2.25, 2.25, np.float32(0.7), 1.25, 1.25]    # 1.5 * (3 / 2); v = 0 -> r = 1; off: passed through
    assert c.tolist() == [-10.0, -10.0, 3.0, 0.0, 0.0] and on.tolist() == [1, 1, 1, 0, 0]


def test_restated_follow2_properties():
    f0 = np.array([[220.0, 440.0, 0.0, 880.0]] * 5, dtype=np.float32)   # pitch -21, -9, 3: mean -9, variance 96
    state = np.zeros((5, 3))
    kw = dict(f0_rate=[1] * 5, offset=[0.5] * 5, auto_on=[1, 0, 0, 0, 1], target=[3.0] * 5, inton=[1.0, 1.0, 1.5, 1.0, 0.5],
              range_on=[0, 0, 0, 1, 1], target_sd=[0.0, 0.0, 0.0, np.sqrt(96.0) / 4, 1e9], emit=[1, 1, 1, 1, 0], decay=1.0, prior=3.0)
    new, shift, it, c, on = RR.follow2_rows(state, f0, **kw)
    assert new[0].tolist() == [-27.0, 3.0, 531.0] and new[1].tolist() == [0.0] * 3 and new[4].tolist() == [0.0] * 3
    # row 0, auto only: the two-moment recurrence's shift, intonation 1, no centre
    _, want = PR.follow_rows(np.zeros((1, 2)), f0[:1], [1], [0.5], [1], [3.0], [1], 1.0, 3.0)
    assert shift[0] == want[0] == np.float32(0.5) + np.float32(6.0) and it[0] == 1.0 and on[0] == 0 and c[0] == -9.0
    # row 1 does not follow; row 4 follows but has heard nothing (not emitting, W == 0): both give offset, 1, 0
    for r in (1, 4):
        assert (shift[r], it[r], c[r], on[r]) == (np.float32(0.5), 1.0, 0.0, 0)
    # row 2, intonation 1.5 at a = 1/2: 1.25, around the mean; row 3, auto range towards a quarter of its sd: 1 + (1/4 - 1) / 2,
    # clamped first to 1 / range_max = 1/2: 1 + (1/2 - 1) / 2
    assert (shift[2], it[2], c[2], on[2]) == (np.float32(0.5), 1.25, -9.0, 1)
    assert (shift[3], it[3], c[3], on[3]) == (np.float32(0.5), 0.75, -9.0, 1)
    # the state is carried, decays, and a not-emitting row forms its outputs from what it has
    new2, _, it2, _, _ = RR.follow2_rows(new, f0, **dict(kw, decay=0.5, emit=[0, 1, 0, 1, 1]))
    assert new2[0].tolist() == new[0].tolist() and new2[3].tolist() == [-40.5, 4.5, 796.5]
    assert it2[2] == it[2] and it2[4] == np.float32(1.0 + 0.5 * (0.5 * 2.0 - 1.0))          # row 4: clamped up to range_max


def test_restated_centred_transform():
    f0 = np.array([[220.0, 440.0, 0.0, 880.0, np.nan, -5.0]] * 4, dtype=np.float32)
    for mode in (0, 1):
        out = RR.transform_rows_centred(f0, mode, [1.0, 0.5, 1.0, 2.0], [0.0, 12.0, 0.0, 0.0], [1.0, 1.0, 0.0, 2.0], [0.0, 0.0, 3.0, -9.0],
                                        [0, 0, 1, 1])
        assert out.dtype == np.float32 and np.all(out[:, [2, 4, 5]] == 0.0)
        assert out[0, [0, 1, 3]].tolist() == [220.0, 440.0, 880.0]     # the identity
        assert out[1, [0, 1, 3]].tolist() == [220.0, 440.0, 880.0]     # an octave up, half the rate
        if mode == 0:
            assert out[2, [0, 1, 3]].tolist() == [880.0] * 3           # intonation 0: everything at the centre
            assert out[3, [0, 1, 3]].tolist() == [220.0, 880.0, 3520.0]     # excursions doubled around 440 Hz, then the rate
        else:                                                          # the rate first: 440, 880, 1760 around 440 doubled
            assert out[2, [0, 1, 3]].tolist() == [880.0] * 3 and out[3, [0, 1, 3]].tolist() == [440.0, 1760.0, 7040.0]


# ------------------------------------------------------------------------------------------------ voices carry a range
class FakeLib:
    @staticmethod
    def alive_library_pack_rows(tok, m, d, rows, norms, stream):
        (ctypes.c_float * m).from_address(norms)[:] = [1.0] * m
        return 0

    @staticmethod
    def alive_pool_append(*a):
        return 0

    @staticmethod
    def alive_pool_move_rows(*a):
        return 0


@pytest.fixture
def host_pool(monkeypatch):
    monkeypatch.setattr(nat, "lib", lambda: FakeLib)
    monkeypatch.setattr(nat, "ptr", lambda t: t.data_ptr())
    monkeypatch.setattr(nat, "stream", lambda: None)
    monkeypatch.setattr(MS.VoicePool, "_changed", lambda self: setattr(self, "mutations", self.mutations + 1))


def test_ranges_merge_on_extend_and_go_with_their_voice(host_pool):
    pool = MS.VoicePool(capacity=256, device="cpu")
    pool.add("a", torch.ones(768, 4), register=(-40.0, 4.0, 416.0))       # mean -10, variance 4
    pool.add("b", torch.ones(768, 3), register=(12.0, 2.0))               # a 2-tuple: as today, no range
    pool.add("c", torch.ones(768, 5))
    assert pool.register("a") == -10.0 and pool.pitch_range("a") == 2.0
    assert pool.register("b") == 6.0 and pool.pitch_range("b") is None and pool.pitch_range("c") is None
    assert pool.registers == {"a": (-40.0, 4.0), "b": (12.0, 2.0)}        # what reads (sum, count) reads what it did
    pool.extend("a", torch.ones(768, 30), register=(-40.0, 4.0, 416.0))   # (the voice moves) all three sums add: variance 104 - 100
    assert pool.registers["a"] == (-80.0, 8.0) and pool.pitch_range("a") == 2.0 and pool.ranges["a"] == 832.0
    pool.extend("a", torch.ones(768, 2))                                  # no register: the voice keeps both
    assert pool.pitch_range("a") == 2.0
    pool.extend("c", torch.ones(768, 2), register=MS.Register(3.0, 1.0, 9.0))     # what measure_register returns
    assert pool.register("c") == 3.0 and pool.pitch_range("c") == 0.0     # one frame: a second moment without variance
    pool.extend("b", torch.ones(768, 2), register=(3.0, 1.0, 9.0))        # the voice's earlier audio has no sum of squares:
    assert pool.registers["b"] == (15.0, 3.0) and pool.pitch_range("b") is None       # the register merges, a range would be wrong
    pool.remove("b")
    pool.compact()
    assert pool.pitch_range("a") == 2.0 and "b" not in pool.ranges
    pool.add("b", torch.ones(768, 3))                                     # back under its name: no stale range
    assert pool.pitch_range("b") is None
    pool.extend("a", torch.ones(768, 1), register=(1.0, 1.0))             # a 2-tuple piece ends the voice's range
    assert pool.registers["a"] == (-79.0, 9.0) and pool.pitch_range("a") is None
    # declared: around a declared register, or around the one the voice has
    pool.set_register("b", hz=880.0, range_st=2.5)
    assert pool.register("b") == 3.0 and abs(pool.pitch_range("b") - 2.5) < 1e-12 and pool.registers["b"] == (3.0, 1.0)
    pool.set_register("b", hz=440.0)                                      # hz alone: the range goes with the old register
    assert pool.register("b") == -9.0 and pool.pitch_range("b") is None
    pool.set_register("a", range_st=4.0)
    assert pool.registers["a"] == (-79.0, 9.0) and abs(pool.pitch_range("a") - 4.0) < 1e-12
    pool.set_register("b", register=(-30.0, 3.0, 312.0))
    assert pool.register("b") == -10.0 and pool.pitch_range("b") == 2.0
    pool.set_register("b")
    assert pool.register("b") is None and pool.pitch_range("b") is None
    assert isinstance(MS.Register(1.0, 2.0, 3.0), tuple) and MS.Register(1.0, 2.0, 3.0) == (1.0, 2.0)
    import copy
    import pickle
    for again in (pickle.loads(pickle.dumps(MS.Register(1.0, 2.0, 3.0))), copy.copy(MS.Register(1.0, 2.0, 3.0)),
                  copy.deepcopy(MS.Register(1.0, 2.0, 3.0))):                # a measured register crosses processes like a tuple
        assert type(again) is MS.Register and again == (1.0, 2.0) and again.sumsq == 3.0
    for bad in (dict(range_st=0.0), dict(range_st=-1.0), dict(range_st=float("nan")), dict(range_st=True),
                dict(hz=100.0, range_st="2"), dict(register=(1.0, 1.0, 1.0), range_st=2.0), dict(register=(1.0, 1.0, -1.0)),
                dict(register=(1.0, 1.0, float("inf"))), dict(register=(1.0, 1.0, 1.0, 1.0))):
        with pytest.raises(ValueError):
            pool.set_register("a", **bad)
    with pytest.raises(ValueError, match="range_st= needs hz= or a voice that has a register"):
        pool.set_register("b", range_st=2.0)
    assert abs(pool.pitch_range("a") - 4.0) < 1e-12
    with pytest.raises(ValueError, match="unknown voice"):
        pool.pitch_range("nobody")


def test_default_pool_takes_three_sums(host_pool):
    pool = MS.VoicePool({"a": torch.ones(768, 2), "b": torch.ones(768, 4)}, device="cpu",
                        registers={"a": (-18.0, 2.0), "b": (-18.0, 2.0, 180.0)})
    assert pool.register("a") == pool.register("b") == -9.0 and pool.pitch_range("a") is None and pool.pitch_range("b") == 3.0
    pool.add("c", torch.ones(768, 3), register=(3.0, 1.0, 25.0))          # re-packs the pool
    assert pool.pitch_range("b") == 3.0 and pool.pitch_range("c") == 4.0


def test_blend_range_is_the_weighted_mean_of_the_standard_deviations(host_pool):
    pool = MS.VoicePool(capacity=32, device="cpu")
    pool.add("a", torch.ones(768, 4), register=(-40.0, 4.0, 416.0))       # sd 2
    pool.add("b", torch.ones(768, 4), register=(6.0, 2.0, 50.0))          # mean 3, variance 16: sd 4
    pool.add("bare", torch.ones(768, 4), register=(6.0, 2.0))
    names, weights = MS.blend_spec([("b", 3), ("a", 1)], pool, 4)
    assert pool.blend_range(names, weights) == weights[0] * 4.0 + weights[1] * 2.0 == 3.5
    assert pool.blend_range(*MS.blend_spec("a", pool, 4)) == 2.0
    with pytest.raises(ValueError, match="voice 'bare' has no pitch range"):
        pool.blend_range(*MS.blend_spec({"a": 1, "bare": 2, "b": 1}, pool, 4))


# ------------------------------------------------------------------------------------------------ the converters' checks
def test_converters_check_their_pitch_range_arguments():
    assert "intonation" in MS._PARAMS and "auto_range" in MS._PARAMS
    with pytest.raises(ValueError, match="MultiStreamConverter: pitch_range must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, pitch_range=1)
    for bad in (0.5, float("inf"), float("nan"), True, "2"):
        with pytest.raises(ValueError, match="MultiStreamConverter: pitch_range_max=.* must be a finite number >= 1"):
            MS.MultiStreamConverter(None, None, None, None, 1, pitch_range=True, pitch_range_max=bad)
    from module.realtime import RealtimeConverter
    for bad in (-0.5, float("inf"), float("nan"), True, "1.5"):
        with pytest.raises(ValueError, match="RealtimeConverter: intonation=.* must be a finite number >= 0"):
            RealtimeConverter(None, None, None, None, intonation=bad)
    with pytest.raises(ValueError, match="intonation_half_life=0 must be > 0"):
        RealtimeConverter(None, None, None, None, intonation=1.5, intonation_half_life=0)
    with pytest.raises(ValueError, match="intonation_prior=-1 must be >= 0"):
        RealtimeConverter(None, None, None, None, intonation=1.5, intonation_prior=-1)
    assert MS.check_intonation(0) == 0.0 and MS.check_range_max(1) == 1.0


# ------------------------------------------------------------------------------------------------ the CLIs' files
@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "spk.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, entries, name="f.json"):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_sessions_file_takes_intonation_auto_range_and_range_st(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, intonation=1.5, auto_range=True, register_hz=180, range_st=2.5),
                                              dict(sess, intonation=1, auto_range=False)]))
    assert set(a) == set(c) == set(MSI.SESSION_KEYS)                  # without the keys, or at their defaults: what it was
    assert (b["intonation"], b["auto_range"], b["range_st"], b["register_hz"]) == (1.5, True, 2.5, 180.0)
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, intonation=1.0), dict(sess, auto_range=False)]), intonation=0.5,
                                auto_range=True)                       # -int / --auto-range: the defaults
    assert (a["intonation"], a["auto_range"]) == (0.5, True) and "intonation" not in b and b["auto_range"] is True
    assert c["intonation"] == 0.5 and "auto_range" not in c
    for bad in (-1, True, "1.5", None, float("nan")):
        with pytest.raises(ValueError, match=r"session 0: \"intonation\"=.* must be a finite number >= 0"):
            MSI.load_sessions(write(files, [dict(sess, intonation=bad)]))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match=r"session 1: \"auto_range\" must be true or false"):
            MSI.load_sessions(write(files, [sess, dict(sess, auto_range=bad)]))
    with pytest.raises(ValueError, match=r"-int / --auto-range: \"intonation\"=-2 must be"):
        MSI.load_sessions(write(files, [sess]), intonation=-2)
    for bad in (0, -3, True, "2"):
        with pytest.raises(ValueError, match=r"session 0: \"range_st\" must be a number of semitones > 0"):
            MSI.load_sessions(write(files, [dict(sess, register_hz=100, range_st=bad)]))
    with pytest.raises(ValueError, match=r"session 0: \"range_st\" declares the pitch range of a voice given by \"lib\" alone"):
        MSI.load_sessions(write(files, [dict(sess, target="spk.wav", range_st=2)]))
    with pytest.raises(ValueError, match=r"session 0: \"range_st\" goes beside \"register_hz\""):
        MSI.load_sessions(write(files, [dict(sess, range_st=2)]))
    ss = MSI.load_sessions(write(files, [dict(sess, register_hz=120, range_st=2), dict(sess, register_hz=120, range_st=2)]))
    name_of = lambda s: MSI.voice_name(s["target"], s["lib"])        # noqa: E731
    assert MSI.declared_ranges(ss, name_of) == {name_of(ss[0]): 2.0}
    ss = MSI.load_sessions(write(files, [dict(sess, register_hz=120, range_st=2), dict(sess, register_hz=120, range_st=3)]))
    with pytest.raises(ValueError, match="earlier entry gave this voice 2"):
        MSI.declared_ranges(ss, name_of)
    with pytest.raises(ValueError, match=r"unknown keys \['range'\]"):
        MSI.load_sessions(write(files, [dict(sess, range=2)]))
    args = MSI.build_parser().parse_args(["s.json"])
    assert args.intonation == 1.0 and args.auto_range is False
    args = MSI.build_parser().parse_args(["s.json", "-int", "1.5", "--auto-range"])
    assert args.intonation == 1.5 and args.auto_range is True


def test_jobs_file_takes_auto_range_and_range_st(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = BI.load_jobs(write(files, [job, dict(job, auto_range=True, register_hz=180, range_st=2.5), dict(job, auto_range=False)]))
    assert set(a) == set(c) == set(BI.JOB_KEYS)
    assert (b["auto_range"], b["range_st"]) == (True, 2.5)
    a, b = BI.load_jobs(write(files, [job, dict(job, auto_range=False)]), auto_range=True)           # --auto-range: the default
    assert a["auto_range"] is True and "auto_range" not in b
    for bad in (1, 0, "true", None):
        with pytest.raises(ValueError, match=r"job 1: \"auto_range\" must be true or false"):
            BI.load_jobs(write(files, [job, dict(job, auto_range=bad)]))
    for bad in (0, -3, True, "2"):
        with pytest.raises(ValueError, match=r"job 0: \"range_st\" must be a number of semitones > 0"):
            BI.load_jobs(write(files, [dict(job, register_hz=100, range_st=bad)]))
    with pytest.raises(ValueError, match=r"job 0: \"range_st\" declares the pitch range of a voice given by \"lib\" alone"):
        BI.load_jobs(write(files, [dict(job, target="spk.wav", range_st=2)]))
    with pytest.raises(ValueError, match=r"job 0: \"range_st\" goes beside \"register_hz\""):
        BI.load_jobs(write(files, [dict(job, range_st=2)]))
    jobs = BI.load_jobs(write(files, [dict(job, register_hz=150, range_st=2), dict(job, input="spk.wav", register_hz=150, range_st=2)]))
    assert BI.declared_ranges(jobs) == {BI.voice_key(jobs[0]): 2.0}
    with pytest.raises(ValueError, match="earlier job gave this voice 2"):
        BI.declared_ranges(BI.load_jobs(write(files, [dict(job, register_hz=150, range_st=2),
                                                      dict(job, register_hz=150, range_st=3)])))
    assert BI.build_parser().parse_args(["j.json"]).auto_range is False
    assert BI.build_parser().parse_args(["j.json", "--auto-range"]).auto_range is True


def test_realtime_cli_takes_int():
    import realtime_inference as RI
    assert RI.build_parser().parse_args([]).intonation == 1.0
    assert RI.build_parser().parse_args(["-int", "1.5"]).intonation == 1.5
