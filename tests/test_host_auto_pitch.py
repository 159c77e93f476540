"""CPU tests of auto pitch: the NumPy restatement (tools/pitch_ref.py) against the reference's own expression (inference.py:119-121,
restated with torch), the follow recurrence's properties, voice registers on the pool's host side (merge on extend, a blend's weighted
target), the C ABI's refusals, and the jobs / sessions files ("auto_pitch" a JSON bool, "register_hz" for a lib-only voice; a file
without the keys parses to the parameters it had)."""
import json
import math
import os
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
import pitch_ref as PR                                               # noqa: E402


def reference_mean_pitch(f0):
    """inference.py:119-121 verbatim in torch on the CPU"""
    f0 = torch.as_tensor(f0, dtype=torch.float32)
    pitch = 12 * torch.log2(f0 / 440) - 9
    return pitch.masked_select(torch.logical_not(torch.logical_or(pitch.isinf(), pitch.isnan()))).mean()


# ------------------------------------------------------------------------------------------------ the restatement
def test_restated_pitch_matches_the_references_expression():
    """Per frame the restatement rounds log2 once from float64 where torch's float32 log2 is within an ulp of |log2| <= 8
    (<= 9.5e-7): times 12 that is 1.2e-5, plus one rounding each of the product and the difference at magnitude <= 128 (<= 7.7e-6
    each): 2.7e-5 per frame, and no more for the mean of frames that agree on which are voiced (they do: 0, negatives, NaN, inf)."""
    rng = np.random.default_rng(5)
    f0 = rng.uniform(40.0, 1100.0, size=(4, 97)).astype(np.float32)
    f0[0, ::3] = 0.0
    f0[1, 5] = np.nan
    f0[1, 9] = np.inf
    f0[2, ::5] = -120.0
    f0[3, :] = 0.0
    p = PR.pitch(f0)
    ref = 12 * torch.log2(torch.from_numpy(f0) / 440) - 9
    assert np.array_equal(PR.voiced(p), torch.isfinite(ref).numpy())
    v = PR.voiced(p)
    assert not v[0, ::3].any() and not v[1, 5] and not v[1, 9] and not v[2, ::5].any() and not v[3].any() and v.sum() > 200
    assert float(np.abs(p[v] - ref.numpy()[v]).max()) <= 2.7e-5
    for row in (f0[0], f0[1], f0[2], f0[:3]):
        assert abs(PR.mean_pitch(row) - float(reference_mean_pitch(row))) <= 2.7e-5
    assert math.isnan(PR.mean_pitch(f0[3])) and bool(torch.isnan(reference_mean_pitch(f0[3])))
    assert PR.pitch(np.float32(440.0)) == np.float32(-9.0) and PR.pitch(np.float32(880.0)) == np.float32(3.0)
    assert MS.pitch_hz(880.0) == 3.0 and MS.pitch_hz(220.0) == -21.0
    assert MS.pitch_hz(123.4) == float(PR.pitch(np.float32(123.4)))


def test_restated_stats_and_offline_shift():
    f0 = np.array([[100.0, 0.0, 200.0, np.nan], [0.0, 0.0, -1.0, np.inf], [440.0, 880.0, 0.0, 220.0]], dtype=np.float32)
    st = PR.stats_groups(f0, [0, 1, 1, 2, 3])
    assert st.shape == (4, 2) and st[:, 1].tolist() == [2.0, 0.0, 0.0, 3.0]
    assert st[1].tolist() == [0.0, 0.0] and st[2].tolist() == [0.0, 0.0]         # an empty group, an all-unvoiced group
    assert st[3, 0] == -9.0 + 3.0 - 21.0
    assert PR.stats_groups(f0, [0, 3], 1, 3)[0].tolist() == [float(PR.pitch(np.float32(200.0))) + 3.0, 2.0]
    shift = PR.shift_groups(st, [1.0, 2.0, 3.0, 0.5], [1, 1, 0, 1], [0.0, 5.0, 5.0, -6.0])
    assert shift.dtype == np.float32
    assert shift[1] == 2.0 and shift[2] == 3.0                                    # nothing voiced / not on auto: the offset alone
    assert shift[3] == np.float32(0.5) + (np.float32(-6.0) - np.float32(-9.0))    # the mean is -9: up three semitones, plus 0.5
    assert shift[0] == np.float32(1.0) + (np.float32(0.0) - np.float32(st[0, 0] / 2.0))


# ------------------------------------------------------------------------------------------------ the follow recurrence
def _follow(f0, n_calls, decay, prior, target=0.0, offset=0.0, rate=1.0, emit=1, auto=1, state=None):
    state = np.zeros((1, 2)) if state is None else state
    shifts = []
    for _ in range(n_calls):
        state, s = PR.follow_rows(state, f0, [rate], [offset], [auto], [target], [emit], decay, prior)
        shifts.append(float(s[0]))
    return state, shifts


def test_follow_recurrence_shrinks_towards_zero_and_never_jumps():
    f0 = np.full((1, 10), 220.0, dtype=np.float32)            # pitch -21 on every frame; the target is 12 above it
    full = -9.0 - -21.0
    state, shifts = _follow(f0, 6, 1.0, 20.0, target=-9.0)
    # decay 1: W = 10 j after j calls, and the shift is W / (W + prior) of the full correction: 1/3, 1/2, 3/5, ...
    assert state[0].tolist() == [-21.0 * 60, 60.0]
    assert np.allclose(shifts, [full * 10 * j / (10 * j + 20.0) for j in range(1, 7)], rtol=0, atol=1e-6)
    assert all(b > a for a, b in zip(shifts, shifts[1:])) and shifts[-1] < full
    # prior 0: the full correction from the first voiced frame on, plus the offset
    _, s0 = _follow(f0, 2, 1.0, 0.0, target=-9.0, offset=1.5)
    assert s0 == [full + 1.5] * 2
    # W == 0 gives exactly the offset, whatever the prior -- 0 included (no 0 / 0)
    silent = np.zeros((1, 10), dtype=np.float32)
    for prior in (0.0, 20.0):
        st, s = _follow(silent, 3, 0.5, prior, target=-9.0, offset=-2.25)
        assert s == [-2.25] * 3 and st[0].tolist() == [0.0, 0.0]
    # a decay forgets: the weight converges to 10 / (1 - decay) and the mean follows a change of register
    st, _ = _follow(f0, 200, 0.5, 20.0)
    assert abs(st[0, 1] - 20.0) < 1e-9
    st, s = _follow(np.full((1, 10), 440.0, dtype=np.float32), 60, 0.5, 0.0, target=-9.0, state=st)
    assert abs(s[-1]) < 1e-6
    # f0_rate enters the pitch (what the mode-1 transform forms): half the rate is an octave down
    _, s = _follow(f0, 1, 1.0, 0.0, target=-21.0, rate=0.5)
    assert s == [12.0]


def test_follow_recurrence_leaves_other_rows_alone():
    f0 = np.full((3, 4), 220.0, dtype=np.float32)
    state = np.array([[5.0, 2.0], [7.0, 3.0], [0.0, 0.0]])
    new, shift = PR.follow_rows(state, f0, [1, 1, 1], [0.1, 0.2, 0.3], [0, 1, 1], [0.0, 0.0, 0.0], [1, 0, 1], 0.9, 1.0)
    assert new[0].tolist() == [5.0, 2.0] and shift[0] == np.float32(0.1)             # not on auto: offset, state untouched
    assert new[1].tolist() == [7.0, 3.0]                                             # not emitting: state stays, the shift is formed
    assert shift[1] == np.float32(0.2) + np.float32(3.0 / 4.0 * (0.0 - 7.0 / 3.0))
    assert new[2].tolist() == [-84.0, 4.0]
    assert PR.decay_of(0.06, None) == 1.0 and PR.decay_of(10.0, 10.0) == 0.5
    assert MS.auto_constants(0.06, 8) == (2.0 ** (-0.06 / 10.0), 0.5 * 50 * 8)
    assert MS.auto_constants(0.01, 16, None, 0.25) == (1.0, 200.0)


# ------------------------------------------------------------------------------------------------ voice registers
class FakeLib:
    @staticmethod
    def alive_library_pack_rows(tok, m, d, rows, norms, stream):
        import ctypes
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


def test_registers_merge_on_extend_and_go_with_their_voice(host_pool):
    pool = MS.VoicePool(capacity=64, device="cpu")
    pool.add("a", torch.ones(768, 4), register=(-40.0, 4.0))
    pool.add("b", torch.ones(768, 3))
    pool.add("c", torch.ones(768, 5), register=(12.0, 2.0))
    assert pool.register("a") == -10.0 and pool.register("b") is None and pool.register("c") == 6.0
    pool.extend("a", torch.ones(768, 30), register=(-8.0, 4.0))          # (does not fit behind a: the voice moves)
    assert pool.registers["a"] == (-48.0, 8.0) and pool.register("a") == -6.0
    pool.extend("a", torch.ones(768, 2))                                  # no register: the voice keeps its own
    pool.extend("b", torch.ones(768, 2), register=(3.0, 1.0))             # a voice without one gets the new audio's
    assert pool.register("a") == -6.0 and pool.register("b") == 3.0
    pool.remove("b")
    pool.compact()
    assert pool.registers == {"a": (-48.0, 8.0), "c": (12.0, 2.0)}
    pool.add("b", torch.ones(768, 3))                                     # back under its name: a new voice, no stale register
    assert pool.register("b") is None
    pool.set_register("b", hz=880.0)
    assert pool.register("b") == 3.0
    pool.set_register("b", register=(-30.0, 3.0))
    assert pool.register("b") == -10.0
    pool.set_register("b")
    assert pool.register("b") is None
    for bad in (dict(hz=0.0), dict(hz=-1.0), dict(hz=float("nan")), dict(hz=True), dict(register=(1.0,)), dict(register=(1.0, -1.0)),
                dict(register=(float("inf"), 1.0)), dict(hz=100.0, register=(1.0, 1.0))):
        with pytest.raises(ValueError):
            pool.set_register("c", **bad)
    assert pool.register("c") == 6.0
    with pytest.raises(ValueError, match="unknown voice"):
        pool.register("nobody")
    with pytest.raises(ValueError, match="unknown voice"):
        pool.set_register("nobody", hz=100.0)
    with pytest.raises(ValueError, match="register"):
        pool.add("d", torch.ones(768, 1), register=(1.0, -2.0))
    assert "d" not in pool.segments
    assert pool.register("a") == -6.0                                     # an all-unvoiced register counts as none
    pool.set_register("a", register=(0.0, 0.0))
    assert pool.register("a") is None


def test_default_pool_keeps_registers_through_a_repack(host_pool):
    pool = MS.VoicePool({"a": torch.ones(768, 2), "b": torch.ones(768, 4)}, device="cpu", registers={"b": (-18.0, 2.0)})
    assert pool.register("a") is None and pool.register("b") == -9.0
    pool.add("c", torch.ones(768, 3), register=(3.0, 1.0))                # re-packs the pool
    assert pool.register("b") == -9.0 and pool.register("c") == 3.0


def test_blend_target_is_the_weighted_mean_in_the_callers_order(host_pool):
    pool = MS.VoicePool(capacity=32, device="cpu")
    pool.add("a", torch.ones(768, 4), register=(-40.0, 4.0))
    pool.add("b", torch.ones(768, 4), register=(6.0, 2.0))
    pool.add("bare", torch.ones(768, 4))
    names, weights = MS.blend_spec([("b", 3), ("a", 1)], pool, 4)
    assert pool.blend_register(names, weights) == weights[0] * 3.0 + weights[1] * -10.0 == 0.75 * 3.0 - 2.5
    assert pool.blend_register(*MS.blend_spec("a", pool, 4)) == -10.0
    with pytest.raises(ValueError, match="voice 'bare' has no register"):
        pool.blend_register(*MS.blend_spec({"a": 1, "bare": 2}, pool, 4))


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_auto_pitch_abi_refuses_bad_arguments():
    L = nat.lib()
    assert L.alive_pitch_stats_groups(None, 1, 1, 0, 1, 16, 1, 16, None) == -1 and b"null" in L.alive_last_error()
    assert L.alive_pitch_stats_groups(16, 1, 1, 0, 1, None, 1, 16, None) == -1 and b"null" in L.alive_last_error()
    for n, t, g in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert L.alive_pitch_stats_groups(16, n, t, 0, 0, 16, g, 16, None) == -1
    for lo, hi in ((-1, 4), (3, 2), (0, 9)):
        assert L.alive_pitch_stats_groups(16, 2, 8, lo, hi, 16, 1, 16, None) == -1 and b"outside [0, 8)" in L.alive_last_error()
    assert L.alive_pitch_shift_groups(16, 16, 1, 1, 16, 16, None, 16, None) == -1 and b"null" in L.alive_last_error()
    assert L.alive_pitch_shift_groups(16, 16, 0, 1, 16, 16, 16, 16, None) == -1
    ok = [16, 2, 8, 16, 16, 16, 16, 16, 0.5, 1.0, 16, 16, None]
    for i in (0, 3, 4, 5, 6, 7, 10, 11):
        a = list(ok)
        a[i] = None
        assert L.alive_pitch_follow_rows(*a) == -1 and b"null" in L.alive_last_error()
    for i, bad in ((1, 0), (2, 0), (8, -0.1), (8, 1.5), (8, float("nan")), (9, -1.0)):
        a = list(ok)
        a[i] = bad
        assert L.alive_pitch_follow_rows(*a) == -1, (i, bad)


# ------------------------------------------------------------------------------------------------ the CLIs' files
def test_auto_pitch_is_a_session_setting():
    assert "auto_pitch" in MS._PARAMS


@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "spk.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, entries, name="f.json"):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_jobs_file_takes_auto_pitch_as_a_bool(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = BI.load_jobs(write(files, [job, dict(job, auto_pitch=True, register_hz=180), dict(job, auto_pitch=False)]))
    assert (a["auto_pitch"], b["auto_pitch"], c["auto_pitch"]) == (False, True, False)
    assert (a["register_hz"], b["register_hz"]) == (None, 180.0)
    a, b = BI.load_jobs(write(files, [job, dict(job, auto_pitch=False)]), auto_pitch=True)         # --auto-pitch: the default
    assert (a["auto_pitch"], b["auto_pitch"]) == (True, False)
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError, match=r"job 1: \"auto_pitch\" must be true or false"):
            BI.load_jobs(write(files, [job, dict(job, auto_pitch=bad)]))
    for bad in (0, -3, True, "180"):
        with pytest.raises(ValueError, match=r"job 0: \"register_hz\" must be a number > 0"):
            BI.load_jobs(write(files, [dict(job, register_hz=bad)]))
    with pytest.raises(ValueError, match=r"job 0: \"register_hz\" declares the register of a voice given by \"lib\" alone"):
        BI.load_jobs(write(files, [dict(job, target="spk.wav", register_hz=150)]))
    with pytest.raises(ValueError, match=r"\"lib\" alone"):
        BI.load_jobs(write(files, [{"input": "a.wav", "blend": [{"lib": "voice_library.pt", "weight": 1}], "register_hz": 150}]))
    jobs = BI.load_jobs(write(files, [dict(job, register_hz=150), dict(job, input="spk.wav", register_hz=150)]))
    assert BI.declared_registers(jobs) == {BI.voice_key(jobs[0]): 150.0}
    with pytest.raises(ValueError, match="earlier job gave this voice 150"):
        BI.declared_registers(BI.load_jobs(write(files, [dict(job, register_hz=150), dict(job, register_hz=151)])))
    # a file without the keys: the parameters it had, plus the two defaults
    plain = BI.load_jobs(write(files, [dict(job, pitch=2, k=3, world_pitch=True)]))[0]
    assert set(plain) == set(BI.JOB_KEYS)
    assert {k: v for k, v in plain.items() if k not in ("auto_pitch", "register_hz")} == dict(
        input=str(files / "a.wav"), target=None, lib=str(files / "voice_library.pt"), output=None, pitch=2.0, intonation=1.0,
        f0_rate=1.0, alpha=0.0, gain=1.0, normalize=False, world_pitch=True, blend=None, k=3)
    assert plain["auto_pitch"] is False and plain["register_hz"] is None
    assert BI.build_parser().parse_args(["j.json"]).auto_pitch is False
    assert BI.build_parser().parse_args(["j.json", "--auto-pitch"]).auto_pitch is True


def test_sessions_file_takes_auto_pitch_as_a_bool(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b = MSI.load_sessions(write(files, [sess, dict(sess, auto_pitch=True, register_hz=97.5, start=2)]))
    assert (a["auto_pitch"], b["auto_pitch"], b["register_hz"], b["start"]) == (False, True, 97.5, 2)
    a, b = MSI.load_sessions(write(files, [sess, dict(sess, auto_pitch=False)]), auto_pitch=True)
    assert (a["auto_pitch"], b["auto_pitch"]) == (True, False)
    for bad in (1, "yes", None, {"on": True}):
        with pytest.raises(ValueError, match=r"session 0: \"auto_pitch\" must be true or false"):
            MSI.load_sessions(write(files, [dict(sess, auto_pitch=bad)]))
    with pytest.raises(ValueError, match=r"session 0: \"register_hz\" must be a number > 0"):
        MSI.load_sessions(write(files, [dict(sess, register_hz=0)]))
    with pytest.raises(ValueError, match=r"session 0: \"register_hz\" declares"):
        MSI.load_sessions(write(files, [dict(sess, target="spk.wav", register_hz=120)]))
    ss = MSI.load_sessions(write(files, [dict(sess, register_hz=120), dict(sess, register_hz=121)]))
    with pytest.raises(ValueError, match="earlier entry gave this voice 120"):
        MSI.declared_registers(ss, lambda s: MSI.voice_name(s["target"], s["lib"]))
    plain = MSI.load_sessions(write(files, [dict(sess, pitch=3, sr=48000)]), k=6)[0]
    assert set(plain) == set(MSI.SESSION_KEYS)
    assert {k: v for k, v in plain.items() if k not in ("auto_pitch", "register_hz")} == dict(
        input=str(files / "a.wav"), target=None, lib=str(files / "voice_library.pt"), output=None, pitch=3.0, f0_rate=1.0, alpha=0.0,
        gain=0.0, input_gain=0.0, start=0, sr=48000, world_pitch=False, blend=None, k=6)
    assert plain["auto_pitch"] is False and plain["register_hz"] is None
    assert MSI.build_parser().parse_args(["s.json"]).auto_pitch is False
    assert MSI.build_parser().parse_args(["s.json", "--auto-pitch"]).auto_pitch is True
