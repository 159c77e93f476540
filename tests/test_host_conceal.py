"""CPU tests of the lost-chunk concealment: the NumPy restatement tools/conceal_ref.py (the period of harmonic signals and their true
continuation, silence, the decay to zeros, the level bound, the recovery, tick by tick against one piece, the lowest-lag tie), the
geometry and every refusal of the converter's host logic, the sessions file and the flags, and the C ABI (symbol, prototype, SRCS,
refusals)."""
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
import conceal_ref as CR                                             # noqa: E402
import multistream_inference as MSI                                  # noqa: E402

R = 16000
G = CR.geometry(R, 160)


def harmonic(P0, n, seed=0, amp=6000.0):
    """an int16 signal of exact integer period P0: the rounding of a periodic signal is periodic"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = sum(a * np.sin(2 * np.pi * h * t / P0 + rng.uniform(0, 6.28)) for h, a in ((1, 1.0), (2, 0.5), (3, 0.25)))
    return np.rint(x * amp).astype(np.int16)


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_constants():
    assert G == dict(lag_lo=40, lag_hi=267, window=320, hold=160, fade=800, recover=80, need=587)
    assert CR.geometry(8000, 80)["need"] == 294 and CR.geometry(44100, 441) == dict(
        lag_lo=110, lag_hi=735, window=882, hold=441, fade=2205, recover=220, need=1617)
    assert CR.geometry(48000, 480, 0, 0, 50)["fade"] == 1 and CR.geometry(48000, 480, 0, 0, 50)["recover"] == 480
    assert (CR.QMAX, CR.MAX_SPAN) == (MS.CONCEAL_QMAX, MS.CONCEAL_MAX_SPAN)
    hdr = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    assert f"#define ALIVE_CONCEAL_MAX_SPAN {CR.MAX_SPAN}\n" in hdr and "#define ALIVE_CONCEAL_QMAX (1 << 30)\n" in hdr
    for rate, cl, b in ((8000, 80, 16), (16000, 160, 4), (44100, 441, 16), (48000, 480, 16)):
        g = CR.geometry(rate, cl)
        assert MS.conceal_geometry(rate, cl, cl * b) == (g["lag_lo"], g["lag_hi"], g["window"], g["hold"], g["fade"], g["recover"])


@pytest.mark.parametrize("P0", [G["lag_lo"] + 1, 100, 160, G["lag_hi"] - 1])
def test_a_harmonic_signal_gives_its_period_and_its_true_continuation(P0):
    x = harmonic(P0, 160 * 40, P0)
    assert np.array_equal(x[:-P0], x[P0:])
    s = CR.StreamRef(R, 160, 16)
    for k in range(30):
        assert np.array_equal(s.feed(x[k * 160:(k + 1) * 160]), x[k * 160:(k + 1) * 160])
    lost = s.feed(None)
    assert s.P == P0 and s.q == 160 == G["hold"]
    assert np.array_equal(lost, x[30 * 160:31 * 160])                # within hold: the true continuation, sample for sample
    assert np.array_equal(s.t, x[30 * 160 - P0:30 * 160])            # (the wrap fade of an exactly periodic ring changes nothing)
    # the lowest-lag tie: lag 2 P0 (if in range) scores exactly what P0 scores
    C, E, sc = CR.scores(x[:30 * 160], G["lag_lo"], G["lag_hi"], G["window"])
    if 2 * P0 <= G["lag_hi"]:
        assert sc[P0 - G["lag_lo"]] == sc[2 * P0 - G["lag_lo"]] == sc.max() and C[P0 - G["lag_lo"]] == E[P0 - G["lag_lo"]]
    assert CR.find_period(x[:30 * 160], G["lag_lo"], G["lag_hi"], G["window"]) == P0


def test_a_silent_ring_gives_the_lowest_lag_and_zeros():
    s = CR.StreamRef(R, 160, 4)
    out = s.feed(None)                                               # a loss at tick 0 on an empty ring
    assert (s.P, s.q) == (G["lag_lo"], 160) and not out.any() and not s.t.any()
    assert not CR.scores(np.zeros(640, np.int16), 40, 267, 320)[2].any()


def test_a_long_loss_decays_to_exact_zeros_and_never_exceeds_the_template():
    rng = np.random.default_rng(3)
    x = np.clip(harmonic(123, 160 * 20, 5, 9000.0) + rng.integers(-800, 800, 160 * 20), -32768, 32767).astype(np.int16)
    s = CR.StreamRef(R, 160, 16)
    for k in range(20):
        s.feed(x[k * 160:(k + 1) * 160])
    outs = [s.feed(None) for _ in range(10)]
    whole = np.concatenate(outs)
    peak = np.abs(s.t.astype(np.int64)).max()
    assert peak > 0 and np.abs(whole.astype(np.int64)).max() <= peak
    end = G["hold"] + G["fade"]
    assert whole[:end - 1].any() and whole[end - 160:end].any() and not whole[end:].any() and len(whole) > end + 300
    assert np.array_equal(CR.att(np.array([0, 160, 161, 560, 959, 960, 5000, CR.QMAX + 500]), 160, 800),
                          [1.0, 1.0, 799 / 800, 0.5, 1 / 800, 0.0, 0.0, 0.0])
    # tick by tick is one piece: the run's samples depend on q alone
    assert np.array_equal(whole, CR.synth(s.t, 0, 1600, G["hold"], G["fade"]))
    assert s.q == 1600 and s.P == len(s.t)
    # the template is taken once: the ring now holds made-up samples and is not searched again
    assert all(np.array_equal(o, CR.synth(s.t, 160 * i, 160, G["hold"], G["fade"])) for i, o in enumerate(outs))
    # saturation far below 2^31
    s.q = CR.QMAX - 10
    s.feed(None)
    assert s.q == CR.QMAX


def test_recovery_fades_the_head_in_and_leaves_the_rest():
    x = harmonic(90, 160 * 24, 7)
    s = CR.StreamRef(R, 160, 16)
    for k in range(20):
        s.feed(x[k * 160:(k + 1) * 160])
    s.feed(None)
    s.feed(None)
    q, t = s.q, s.t.copy()
    c = np.random.default_rng(8).integers(-32768, 32768, 160).astype(np.int16)
    out = s.feed(c)
    rec = G["recover"]
    assert np.array_equal(out[rec:], c[rec:]) and not np.array_equal(out[:rec], c[:rec]) and (s.q, s.P) == (0, 0)
    cont = t.astype(np.float64)[(q + np.arange(rec)) % len(t)] * CR.att(q + np.arange(rec), G["hold"], G["fade"])
    want = np.rint(cont + ((c[:rec] - cont) * np.arange(1, rec + 1)) / (rec + 1))
    assert np.array_equal(out[:rec], want.astype(np.int16))
    lo, hi = np.minimum(cont, c[:rec]) - 1, np.maximum(cont, c[:rec]) + 1
    assert np.all(out[:rec] >= lo) and np.all(out[:rec] <= hi)       # between the two signals
    assert np.array_equal(s.feed(c), c)                              # the run is over: the next chunk goes through
    # full-scale inputs stay int16
    t2 = np.full(50, -32768, np.int16)
    assert CR.recover(t2, 10, np.full(160, 32767, np.int16), 80, 160, 800).dtype == np.int16
    assert np.array_equal(CR.synth(t2, 0, 100, 160, 800), np.full(100, -32768, np.int16))


def test_concealment_off_is_a_chunk_of_zeros():
    x = harmonic(100, 160 * 20, 9)
    s = CR.StreamRef(R, 160, 16, on=False)
    for k in range(18):
        s.feed(x[k * 160:(k + 1) * 160])
    assert not s.feed(None).any() and (s.q, s.P) == (0, 0)
    assert np.array_equal(s.feed(x[18 * 160:19 * 160]), x[18 * 160:19 * 160])


def test_conceal_rows_moves_only_the_rows_that_are_lost_or_recovering():
    rng = np.random.default_rng(11)
    n, ld, ldc, ldt = 6, 2560, 160, 272
    ring = np.stack([harmonic(60 + 20 * r, ld, r) for r in range(n)])
    chunks = rng.integers(-32768, 32768, (n, ldc)).astype(np.int16)
    g = CR.geometry(R, 160)
    k = {a: [g[a]] * n for a in ("lag_lo", "lag_hi", "window", "hold", "fade")}
    args = dict(ring=ring, ring_len=[2560, 2560, 2560, 2560, 2560, 586], chunks=chunks, chunk_len=[160] * n,
                present=[1, 1, 0, 1, 1, 1], lost=[1, 0, 1, 1, 1, 1], on=[1, 1, 1, 0, 1, 1], recover_len=[g["recover"]] * n,
                state=np.array([[0, 0], [0, 0], [0, 0], [0, 0], [320, 77], [0, 0]], np.int32),
                tmpl=rng.integers(-3000, 3000, (n, ldt)).astype(np.int16), **k)
    out = CR.conceal_rows(**args)
    assert out["state"].tolist() == [[160, 60], [0, 0], [0, 0], [0, 0], [480, 77], [0, 0]]
    for r in (1, 2, 5):                                              # real and not in a run; absent; a ring one sample too short
        assert np.array_equal(out["chunks"][r], chunks[r]) and np.array_equal(out["tmpl"][r], args["tmpl"][r])
    assert not out["chunks"][3].any() and np.array_equal(out["tmpl"][3], args["tmpl"][3])
    assert np.array_equal(out["chunks"][0], ring[0, 40:200]) and np.array_equal(out["tmpl"][0, :60], ring[0, 40:100])      # (2560 = 40 mod 60)
    assert np.array_equal(out["chunks"][4], CR.synth(args["tmpl"][4, :77], 320, 160, 160, 800))
    args.update(chunks=out["chunks"], state=out["state"], tmpl=out["tmpl"], lost=[0] * n, present=[1] * n)
    rec = CR.conceal_rows(**args)
    assert rec["state"].tolist() == [[0, 0]] * n and np.array_equal(rec["chunks"][1:4], out["chunks"][1:4])
    assert np.array_equal(rec["chunks"][0, 80:], out["chunks"][0, 80:]) and np.array_equal(rec["tmpl"], out["tmpl"])


# ------------------------------------------------------------------------------------------------ the host logic
def test_geometry_and_its_refusals():
    assert MS.conceal_geometry(16000, 160, 640) == (40, 267, 320, 160, 800, 80)          # -c 160 -b 4 just fits
    with pytest.raises(ValueError, match=r"needs a ring of at least 587 samples .* holds 480"):
        MS.conceal_geometry(16000, 160, 480)
    assert MS.conceal_geometry(16000, 160, 480, check=False)[:3] == (40, 267, 320)
    with pytest.raises(ValueError, match=r"needs a ring of at least 1617 samples .* holds 882"):
        MS.conceal_geometry(44100, 441, 882)
    with pytest.raises(ValueError, match=r"would search 5280 samples .* at most 4096"):
        MS.conceal_geometry(144000, 1440, 1440 * 16)
    for name, kw in (("conceal_hold_ms", dict(hold_ms=-1)), ("conceal_fade_ms", dict(fade_ms=float("nan"))),
                     ("conceal_recover_ms", dict(recover_ms="5")), ("conceal_hold_ms", dict(hold_ms=True))):
        with pytest.raises(ValueError, match=name + r"=.* must be a finite number of milliseconds >= 0"):
            MS.conceal_geometry(16000, 160, 2560, **kw)
    assert MS.conceal_geometry(16000, 160, 2560, 0, 0, 1000)[3:] == (0, 1, 160)
    assert MS.check_conceal_ms() == (10.0, 50.0, 5.0)


def _host_converter(conceal, open_slots=(0, 2), slots=4):
    """the part of a converter the validation of `lost` and of a session's switch reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.conceal, c.B = conceal, slots
    c.is_open = [s in open_slots for s in range(slots)]
    return c


def test_the_converter_refuses_what_it_cannot_do():
    assert "conceal" in MS._PARAMS and MS.MultiStreamConverter.conceal is False
    with pytest.raises(ValueError, match="conceal=True needs sparse=True"):
        MS.MultiStreamConverter(None, None, None, None, 1, conceal=True)
    with pytest.raises(ValueError, match="conceal must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, sparse=True, conceal=1)
    with pytest.raises(ValueError, match=r"MultiStreamConverter: conceal_fade_ms=-5 must be"):
        MS.MultiStreamConverter(None, None, None, None, 1, sparse=True, conceal=True, conceal_fade_ms=-5)
    on, off = _host_converter(True), _host_converter(False)
    assert on._lost_slots({0: 1}, [2]) == [2] and on._lost_slots({}, (2, 0, 2)) == [0, 2] and on._lost_slots({0: 1}, ()) == []
    assert off._lost_slots({0: 1}, ()) == [] and off._lost_slots({}, None) == []
    with pytest.raises(ValueError, match=r"slot 2 is named in both chunks and lost"):
        on._lost_slots({2: 1, 0: 1}, [2])
    with pytest.raises(ValueError, match=r"a lost chunk for slot 1, which is not open"):
        on._lost_slots({0: 1}, [1])
    with pytest.raises(ValueError, match=r"slot 4 out of range"):
        on._lost_slots({}, [4])
    with pytest.raises(ValueError, match=r"lost=\) needs a converter built with MultiStreamConverter\(..., sparse=True, conceal=True\)"):
        off._lost_slots({}, [0])
    assert off._session_conceal(0, dict(conceal=None)) is None and off._session_conceal(0, dict(conceal=False)) is None
    with pytest.raises(ValueError, match=r"slot 3: conceal=True needs a converter built with"):
        off._session_conceal(3, dict(conceal=True))
    for conv in (on, off):
        with pytest.raises(ValueError, match=r"slot 1: conceal must be a bool or None"):
            conv._session_conceal(1, dict(conceal="yes"))
    with pytest.raises(ValueError, match=r"conceal_state needs a converter built with"):
        off.conceal_state()
    # a session's ring against its search, through the converter's own arithmetic
    on.rate, on.buffersize, on._rt, on.chunk, on._conceal_ms = [16000] * 4, 3, None, 160, (10.0, 50.0, 5.0)
    with pytest.raises(ValueError, match=r"slot 0: concealment at 16000 Hz needs a ring of at least 587 samples .* holds 480"):
        on._session_conceal(0, dict(conceal=True))
    with pytest.raises(ValueError, match=r"slot 0: .* at least 587 .* holds 480"):
        on._session_conceal(0, {})                                   # (the converter's default is on)
    assert on._session_conceal(0, dict(conceal=False)) == (False, (40, 267, 320, 160, 800, 80))
    on.buffersize = 4
    assert on._session_conceal(0, {}) == (True, (40, 267, 320, 160, 800, 80))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_symbol_is_exported_and_the_prototype_agrees_with_the_header():
    L = ctypes.CDLL(nat.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    name = "alive_conceal_rows"
    assert hasattr(L, name)
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert decl is not None, f"{name} is not declared in alive_vc.h"
    args = decl.group(1).split(",")
    assert len(args) == 20 == len(nat.PROTOTYPES[name][1]) and nat.PROTOTYPES[name][0] is ctypes.c_int
    assert [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args] == nat.PROTOTYPES[name][1]
    mk = open(os.path.join(ROOT, "alive-vc_amd", "csrc", "Makefile")).read()
    assert "conceal.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]
    assert "-ffp-contract=off" in mk


def test_the_abi_refuses_null_pointers_and_bad_arguments():
    L = nat.lib()
    #     ring  N  ld   rl    chunks ldc cl    pres  lost  on    lo    hi    win   hold  fade  rec   state tmpl  ldt stream
    ok = [4096, 2, 640, 8192, 12288, 160, 8200, 8208, 8216, 8224, 8232, 8240, 8248, 8256, 8264, 8272, 8280, 16384, 272, None]
    for i in (0, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17):
        a = list(ok)
        a[i] = None
        assert L.alive_conceal_rows(*a) == -1 and b"null" in L.alive_last_error(), i
    for i, bad in ((1, 0), (1, -1), (2, 0), (2, -5), (5, 0), (5, -1), (5, 1 << 30), (18, 0), (18, -1)):
        a = list(ok)
        a[i] = bad
        assert L.alive_conceal_rows(*a) == -1 and b"bad args" in L.alive_last_error(), (i, bad)


# ------------------------------------------------------------------------------------------------ the file and the flags
@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "spk.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, entries, name="f.json"):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_sessions_file_takes_lose_and_conceal_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    assert MSI.LOSE_KEYS == ("lose",) and MSI.CONCEAL_KEYS == ("conceal",)
    a, b, c, d, e = MSI.load_sessions(write(files, [sess, dict(sess, lose=[7, 3, 20]), dict(sess, lose=[]), dict(sess, lose=None),
                                                    dict(sess, conceal=False, lose=[1], stall=[0, 2])]))
    assert set(a) == set(MSI.SESSION_KEYS) == set(d) and b["lose"] == (3, 7, 20) and c["lose"] == ()
    assert set(b) == set(MSI.SESSION_KEYS) | {"lose"} and e["conceal"] is False and e["lose"] == (1,) and e["stall"] == (0, 2)
    assert MSI.load_sessions(write(files, [dict(sess, conceal=True)]))[0]["conceal"] is True
    assert "conceal" not in MSI.load_sessions(write(files, [dict(sess, conceal=None)]))[0]
    for bad in (5, [1, 1], [-1], [1.0], [True], "3", {"t": 1}):
        with pytest.raises(ValueError, match=r"session 1: \"lose\""):
            MSI.load_sessions(write(files, [sess, dict(sess, lose=bad)]))
    with pytest.raises(ValueError, match=r"session 0: ticks \[4, 9\] are named in both \"lose\" and \"stall\""):
        MSI.load_sessions(write(files, [dict(sess, lose=[9, 4, 2], stall=[4, 5, 9])]))
    for bad in (1, "true", [True]):
        with pytest.raises(ValueError, match=r"session 0: \"conceal\" must be true or false"):
            MSI.load_sessions(write(files, [dict(sess, conceal=bad)]))
    with pytest.raises(ValueError, match=r"--conceal-hold / --conceal-fade / --conceal-recover: conceal_fade_ms=-1 must be"):
        MSI.load_sessions(write(files, [sess]), conceal_fade_ms=-1)
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['lost'\]"):
        MSI.load_sessions(write(files, [dict(sess, lost=[1])]))


def test_the_cli_takes_the_conceal_flags():
    args = MSI.build_parser().parse_args(["s.json"])
    assert (args.conceal, args.conceal_hold, args.conceal_fade, args.conceal_recover) == (False, 10.0, 50.0, 5.0)
    args = MSI.build_parser().parse_args(["s.json", "--conceal", "--conceal-hold", "20", "--conceal-fade", "30", "--conceal-recover", "2.5"])
    assert (args.conceal, args.conceal_hold, args.conceal_fade, args.conceal_recover) == (True, 20.0, 30.0, 2.5)


class _Recorder:
    """a converter that only records what run() asks of it"""

    def __init__(self):
        self.calls = []

    def open(self, i, **p):
        self.calls.append(("open", i))

    def close(self, i):
        self.calls.append(("close", i))

    def step(self, feed, lost=None):
        self.calls.append(("step", sorted(feed), lost))
        return {s: None for s in list(feed) + list(lost or [])}


def test_run_drops_the_lost_chunks_and_keeps_the_clock():
    pcm = [np.arange(40, dtype=np.int16), np.arange(30, dtype=np.int16)]
    conv = _Recorder()
    MSI.run(conv, pcm, [0, 1], 10, [{}, {}], loses=[(1, 2, 9), None], stalls=[None, (2,)])
    steps = [c for c in conv.calls if c[0] == "step"]
    # session 0 supplies at ticks 0..3, loses 1 and 2 (9 is beyond its life); session 1 supplies at 1, 3, 4
    assert steps == [("step", [0], None), ("step", [1], [0]), ("step", [], [0]), ("step", [0, 1], None), ("step", [1], None)]
    plain = _Recorder()
    MSI.run(plain, pcm, [0, 1], 10, [{}, {}])
    assert all(c[2] is None for c in plain.calls if c[0] == "step") and len([c for c in plain.calls if c[0] == "step"]) == 4
