"""CPU tests of sparse ticks: the NumPy restatement tools/ring_ref.py (a session's ring is the last `buffersize` chunks it supplied
under any absence pattern; absent and non-fitting rows untouched; the masked row arrays; the two int16 edges), the sessions file's
"stall" and the schedule it gives, the --sparse flag, the constructor's check, the dense converter's refusal of a missing slot without
a device, and the C ABI (symbols, prototypes, refusals)."""
import ctypes
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
import ring_ref as RR                                                # noqa: E402
import multistream_inference as MSI                                  # noqa: E402

GEOM = [(80, 16), (160, 16), (441, 16), (480, 16), (160, 2), (1, 5)]  # (chunk_len, buffersize) per row


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "one", "random"])
def test_a_ring_is_the_last_chunks_its_session_supplied_under_any_absence_pattern(pattern):
    n = len(GEOM)
    cl = [c for c, _ in GEOM]
    rl = [c * b for c, b in GEOM]
    ld, ld_chunk, ld_x = max(rl) + 3, max(cl) + 1, max(rl) + 5
    rng = np.random.default_rng(7)
    ring = np.zeros((n, ld), np.int16)
    x = np.full((n, ld_x), 9.0, np.float32)                           # (a value no push writes)
    seg = np.arange(1, 2 * n + 1, dtype=np.int32)
    world = np.array([1, 0, 1, 1, 0, 1], np.int32)
    supplied = [[] for _ in range(n)]
    for tick in range(2 * 16 + 3):
        present = {"all": [1] * n, "none": [0] * n, "alternating": [(tick + r) % 2 for r in range(n)],
                   "one": [int(r == 2) for r in range(n)], "random": list(rng.integers(0, 2, n))}[pattern]
        chunks = rng.integers(-32768, 32768, (n, ld_chunk)).astype(np.int16)
        before = ring.copy(), x.copy()
        out = RR.push_rows(ring, chunks, cl, rl, present, x, seg, 2, world)
        ring, x = out["ring"], out["x"]
        for r in range(n):
            if present[r]:
                supplied[r].append(chunks[r, :cl[r]].copy())
                assert np.array_equal(x[r, :rl[r]], ring[r, :rl[r]].astype(np.float32) / np.float32(32768)) and not x[r, rl[r]:].any()
            else:
                assert np.array_equal(ring[r], before[0][r]) and np.array_equal(x[r], before[1][r])
            assert np.array_equal(ring[r, :rl[r]], RR.session_ring(supplied[r], GEOM[r][1], cl[r])) and not ring[r, rl[r]:].any()
        assert out["seg_len_tick"].tolist() == [int(v) * int(present[i // 2]) for i, v in enumerate(seg)]
        assert out["world_tick"].tolist() == [int(w) * int(p) for w, p in zip(world, present)]
    if pattern in ("all", "alternating"):                             # every ring turned over: more than twice, and more than once
        assert all(len(s) > (2 if pattern == "all" else 1) * b for s, (_, b) in zip(supplied, GEOM))


def test_rows_whose_lengths_do_not_fit_are_absent_and_the_masks_are_optional():
    ring = np.arange(24, dtype=np.int16).reshape(3, 8)
    x = np.full((3, 8), 5.0, np.float32)
    chunks = np.full((3, 4), -1, np.int16)
    out = RR.push_rows(ring, chunks, [2, 5, 3], [6, 8, 2], [1, 1, 1], x, [7, 8, 9])     # row 1: cl > ld_chunk; row 2: cl > rl
    assert out["ring"][0].tolist() == [2, 3, 4, 5, -1, -1, 6, 7] and out["x"][0, 6:].tolist() == [0.0, 0.0]
    assert np.array_equal(out["ring"][1:], ring[1:]) and np.array_equal(out["x"][1:], x[1:])
    assert out["seg_len_tick"].tolist() == [7, 0, 0] and out["world_tick"] is None
    assert RR.push_rows(ring, chunks, [2, 2, 2], [6, 6, 6], [0, 0, 0], x)["seg_len_tick"] is None
    assert not RR.fits(1, 9, 8, 4, 9) and not RR.fits(1, 9, 9, 4, 8) and not RR.fits(-1, 4, 8, 4, 8) and RR.fits(0, 0, 8, 4, 8)


def test_the_int16_edges_of_the_restatement():
    v = np.array([0.0, 1.0, -1.0, 1.5, -3.0, 0.99999, -0.5 / 32768, 32767.9 / 32768, 1e-40], np.float32)
    assert RR.float_to_pcm16(v).tolist() == [0, -32768, -32768, -16384, -32768, 32767, 0, 32767, 0]
    wave = np.tile(v, (3, 1))
    out = RR.emit_rows(wave, [2, 0, 5], [4, 9, 5], [1, 0, 1], 6)       # row 1 not taken; row 2's span leaves the wave
    assert out.tolist() == [[-32768, -16384, -32768, 32767, 0, 0], [0] * 6, [0] * 6] and out.dtype == np.int16
    assert not RR.emit_rows(wave[:1], [0], [7], [1], 6)[0].any()          # longer than the output row
    assert RR.session_ring([], 3, 2).tolist() == [0] * 6
    assert RR.session_ring([np.array([1, 2]), np.array([3, 4])], 3, 2).tolist() == [0, 0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ the sessions file and the CLI
def _write(d, sessions):
    p = d / "s.json"
    json.dump(sessions, open(p, "w"))
    return str(p)


def test_stall_is_validated_on_the_host_and_kept_only_where_given(tmp_path):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    assert MSI.session_stall({}, "s") is None and MSI.session_stall({"stall": None}, "s") is None
    assert MSI.session_stall({"stall": []}, "s") == () and MSI.session_stall({"stall": [7, 0, 3]}, "s") == (0, 3, 7)
    for bad in (3, "3", [1.0], [True], [-1], [2, "x"], {"a": 1}, [[1]]):
        with pytest.raises(ValueError, match=r"session 1: \"stall\" must be a list of distinct integers >= 0"):
            MSI.load_sessions(_write(tmp_path, [sess, dict(sess, stall=bad)]))
    with pytest.raises(ValueError, match=r"session 0: \"stall\" names a tick twice"):
        MSI.load_sessions(_write(tmp_path, [dict(sess, stall=[4, 2, 4])]))
    a, b = MSI.load_sessions(_write(tmp_path, [sess, dict(sess, stall=[9, 2], start=1)]))
    assert "stall" not in a and set(a) == set(MSI.SESSION_KEYS) and b["stall"] == (2, 9) and "stall" in MSI.STALL_KEYS
    with pytest.raises(ValueError, match="unknown keys"):
        MSI.load_sessions(_write(tmp_path, [dict(sess, stalls=[1])]))
    assert MSI.build_parser().parse_args(["s.json"]).sparse is False
    assert MSI.build_parser().parse_args(["s.json", "--sparse"]).sparse is True
    assert "\"stall\"" in MSI.__doc__ and "--sparse" in MSI.__doc__


def test_a_stalled_session_supplies_its_chunks_later_and_in_order():
    assert MSI.supply_ticks(3, 4) == [3, 4, 5, 6] == MSI.supply_ticks(3, 4, ()) == MSI.supply_ticks(3, 4, (0, 1, 2, 7))
    assert MSI.supply_ticks(3, 4, (3, 4, 6)) == [5, 7, 8, 9] and MSI.supply_ticks(0, 0, (0,)) == []
    assert MSI.supply_ticks(2, 3, (4,)) == [2, 3, 5]


class _Recorder:
    """stands in for a converter: what run() opens, feeds and closes, tick by tick"""

    def __init__(self):
        self.log, self.open_slots = [], set()

    def open(self, slot, **p):
        self.open_slots.add(slot)

    def close(self, slot):
        self.open_slots.discard(slot)
        self.log.append(("close", slot))

    def step(self, feed):
        assert set(feed) <= self.open_slots
        self.log.append({s: c.tolist() for s, c in feed.items()})
        return {s: c.copy() for s, c in feed.items()}


def test_run_moves_a_stalled_sessions_input_later_and_closes_it_after_its_last_chunk():
    pcms = [np.arange(6, dtype=np.int16), np.arange(10, 16, dtype=np.int16)]
    plain, stalled = _Recorder(), _Recorder()
    want = MSI.run(plain, pcms, [0, 1], 2, [{}, {}])
    got = MSI.run(stalled, pcms, [0, 1], 2, [{}, {}], stalls=[(1, 2), None])
    assert all(np.array_equal(a, b) for a, b in zip(want, got)) and np.array_equal(got[0], pcms[0])
    assert plain.log == [{0: [0, 1]}, {0: [2, 3], 1: [10, 11]}, {0: [4, 5], 1: [12, 13]}, ("close", 0), {1: [14, 15]}, ("close", 1)]
    assert stalled.log == [{0: [0, 1]}, {1: [10, 11]}, {1: [12, 13]}, {0: [2, 3], 1: [14, 15]}, ("close", 1), {0: [4, 5]}, ("close", 0)]


def test_run_without_stalls_treats_a_session_without_a_chunk_as_it_always_did():
    """a session whose input is shorter than one chunk never opens, still counts up to its start tick for before / after, and is
    "closed" on the tick before its start (closing a slot that is not open changes nothing)"""
    pcms = [np.arange(4, dtype=np.int16), np.arange(1, dtype=np.int16)]
    rec, ticks = _Recorder(), []
    outs = MSI.run(rec, pcms, [0, 5], 2, [{}, {}], before=ticks.append)
    assert ticks == [0, 1, 2, 3, 4] and len(outs[1]) == 0 and np.array_equal(outs[0], pcms[0])
    assert rec.log == [{0: [0, 1]}, {0: [2, 3]}, ("close", 0), {}, {}, {}, ("close", 1)]
    rec, ticks = _Recorder(), []
    MSI.run(rec, pcms[1:], [0], 2, [{}], before=ticks.append)        # start 0: no tick at all
    assert ticks == [] and rec.log == []


# ------------------------------------------------------------------------------------------------ the converter, without a device
def test_sparse_must_be_a_bool_and_a_dense_converter_still_refuses_a_missing_slot():
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="MultiStreamConverter: sparse must be a bool"):
            MS.MultiStreamConverter(None, None, None, None, 1, sparse=bad)
    assert MS.MultiStreamConverter.sparse is False
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)     # a dense converter's host state: step() refuses before any device work
    c.B, c.is_open = 3, [True, False, True]
    with pytest.raises(ValueError, match=r"open slots \[2\] supplied no chunk this tick"):
        c.step({0: np.zeros(160, np.int16)})
    with pytest.raises(ValueError, match=r"open slots \[0, 2\] supplied no chunk this tick"):
        c.step({})
    with pytest.raises(ValueError, match="a chunk for slot 1, which is not open"):
        c.step({1: np.zeros(160, np.int16)})
    with pytest.raises(ValueError, match="rings needs a converter built with"):
        c.rings()
    c.sparse = True                                                   # a sparse one checks its chunks before anything moves
    c.slot_chunk, c.rate, c.count = [160, 160, 441], [16000, 16000, 44100], [4, 0, 4]
    with pytest.raises(ValueError, match="a chunk for slot 1, which is not open"):
        c.step({1: np.zeros(160, np.int16)})
    with pytest.raises(ValueError, match=r"slot 2: chunk of 440 samples, expected 441 \(the session runs at 44100 Hz\)"):
        c.step({0: np.zeros(160, np.int16), 2: np.zeros(440, np.int16)})
    assert c.count == [4, 0, 4] and c.step({}) == {}


def test_the_push_wrapper_refuses_views_and_wrong_dtypes_before_anything_is_launched():
    import torch
    i32, n = torch.int32, 3
    ring, chunks, x = torch.zeros(n, 16, dtype=torch.int16), torch.zeros(n, 8, dtype=torch.int16), torch.zeros(n, 16)
    cl, rl, pr = torch.zeros(n, dtype=i32), torch.zeros(n, dtype=i32), torch.zeros(n, dtype=torch.uint8)
    seg, w = torch.zeros(2 * n, dtype=i32), torch.zeros(n, dtype=i32)
    for kw, msg in ((dict(ring=ring[:, :8]), "ring must be contiguous"), (dict(chunks=chunks[:, ::2]), "chunks must be contiguous"),
                    (dict(x=x[:, 1:]), "x must be contiguous"), (dict(x=x.double()), "x must be contiguous float32"),
                    (dict(present=pr[:2]), r"present must be \[N\] bytes"), (dict(chunk_len=cl.long()), r"chunk_len must be int32 \[3\]"),
                    (dict(seg_len=seg[:n]), r"seg_len must be int32 \[6\]"), (dict(seg_len_tick=seg.float()), "seg_len_tick must be int32"),
                    (dict(world_on=w[:2]), r"world_on must be int32 \[3\]"), (dict(world_tick=w.long()), "world_tick must be int32"),
                    (dict(seg_len_tick=None), ".*given in pairs"), (dict(world_on=None), ".*given in pairs")):
        args = dict(ring=ring, chunks=chunks, chunk_len=cl, ring_len=rl, present=pr, x=x, seg_len=seg, seg_len_tick=seg.clone(), S=2,
                    world_on=w, world_tick=w.clone())
        args.update(kw)
        with pytest.raises(ValueError, match="ring_push_rows_: " + msg):
            MS.ring_push_rows_(**args)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_library_exports_the_two_entry_points_and_refuses_bad_arguments():
    L = nat.lib()
    hdr = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    for name in ("alive_ring_push_rows", "alive_emit_rows"):
        assert hasattr(L, name) and name in nat.PROTOTYPES and f"int {name}(" in hdr
    one = ctypes.c_void_p(16)                                         # (never dereferenced: every call below is refused first)
    push = lambda *a: L.alive_ring_push_rows(*a)                      # noqa: E731
    ok = [one, 2, 8, one, 8, one, one, one, one, 8, 1, None, None, None, None, None]
    for at, bad in ((0, None), (3, None), (8, None), (1, 0), (2, 0), (4, 0), (9, 0), (10, 0), (11, one), (13, one)):
        args = list(ok)
        args[at] = bad
        assert push(*args) != 0 and b"alive_ring_push_rows" in L.alive_last_error()
    okay = [one, 2, 8, one, one, one, one, 8, None]
    for at, bad in ((0, None), (6, None), (1, 0), (1, 65536), (2, 0), (7, 0), (7, 1 << 30)):
        args = list(okay)
        args[at] = bad
        assert L.alive_emit_rows(*args) != 0 and b"alive_emit_rows" in L.alive_last_error()
