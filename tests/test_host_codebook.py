"""Voice codebooks, the parts that need no GPU: the NumPy restatement (tools/codebook_ref.py) against exact rational arithmetic, the
argument checks of the C entry points (csrc/codebook.hip) and of build_codebook, and the "codebook" key of the sessions file."""
import json
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import codebook_ref as CR                                            # noqa: E402
import multistream_inference as MSI                                  # noqa: E402
from module import _native as nat                                    # noqa: E402
from module import codebook as CB                                    # noqa: E402


# ---------------------------------------------------------------------------------------------------- the restatement
def _round_f32(q):
    """the Fraction q rounded to the nearest float32 (the test's data never lands on a tie)"""
    f = np.float32(float(q))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    dist = [abs(Fraction(float(c)) - q) for c in cands]
    best = min(range(3), key=lambda i: dist[i])
    assert sorted(dist)[0] < sorted(dist)[1], "a tie: choose other data"
    return cands[best]


@pytest.mark.parametrize("n", [1, 513, 2000])
def test_chunked_sequential_mean_is_the_exact_mean_rounded_once(n):
    """rows spread over 2^-24 .. 2^24: the float64 accumulator holds every partial sum of float32 rows of this spread closely enough
    that the mean, rounded to float32 once, is the exact rational mean's rounding -- in the fixed order and in math.fsum's"""
    rng = np.random.RandomState(100 + n)
    x = (rng.randn(n, 6) * np.exp2(rng.randint(-24, 25, size=(n, 1)))).astype(np.float32)
    got = CR.chunked_mean(x)
    assert got.dtype == np.float32 and got.shape == (6,)
    for d in range(6):
        exact = sum((Fraction(float(v)) for v in x[:, d]), Fraction(0)) / n
        assert got[d] == _round_f32(exact), (n, d)
        assert got[d] == np.float32(math.fsum(float(v) for v in x[:, d]) / n), (n, d)


def test_update_takes_members_in_row_order_and_keeps_empty_clusters():
    rng = np.random.RandomState(3)
    rows = rng.randn(40, 5).astype(np.float32)
    assign = np.array([2, 0, 2, 2, 0] * 8)
    cent = np.full((4, 5), 7.25, dtype=np.float32)
    out = CR.update(rows, assign, cent)
    assert np.array_equal(out[1], cent[1]) and np.array_equal(out[3], cent[3])
    assert np.array_equal(out[0], CR.chunked_mean(rows[assign == 0])) and np.array_equal(out[2], CR.chunked_mean(rows[assign == 2]))
    assert np.array_equal(cent, np.full((4, 5), 7.25, dtype=np.float32))          # the input is not written


def test_assignment_breaks_exact_ties_to_the_lowest_index():
    rng = np.random.RandomState(4)
    cent = rng.randn(5, 16).astype(np.float32)
    cent[3] = cent[1]                                                 # an exact duplicate: rows nearest to it tie
    cent[4] = cent[0]
    rows = np.concatenate([cent + 0.01 * rng.randn(5, 16).astype(np.float32), cent]).astype(np.float32)
    a, best, gap = CR.assign_rows(rows, cent, with_gap=True)
    assert a.tolist() == [0, 1, 2, 1, 0, 0, 1, 2, 1, 0]
    assert gap[2] > 0 and all(gap[i] == 0 for i in (0, 1, 3, 4, 5, 6, 8, 9))
    assert np.all(best > 0.99)


def test_stats_sum_order_and_moved():
    rng = np.random.RandomState(5)
    for m in (1, 1023, 1024, 5000):
        v = rng.rand(m).astype(np.float32)
        s = CR.stats_sum(v)
        assert abs(s - math.fsum(float(x) for x in v)) <= 1e-12 * s
    assert CR.moved([1, 2, 3]) == 3 and CR.moved([1, 2, 3], [1, 0, 3]) == 1


def test_restated_build_on_planted_clusters():
    rng = np.random.RandomState(6)
    dirs = rng.randn(3, 768)
    dirs *= 8.0 / np.linalg.norm(dirs, axis=1, keepdims=True)
    label = np.array([0] * 5 + [1] * 9 + [2] * 1)
    rows = ((dirs[label] + 0.05 * rng.randn(15, 768)) * np.exp2(rng.randint(-3, 4, size=(15, 1)))).astype(np.float32)
    st = {}
    book = CR.build_codebook(rows.T, 3, init=[0, 5, 14], stats=st)
    assert st["moved"] == [15, 0] and st["iterations"] == 2 and st["converged"] and st["empty_clusters"] == 0
    assert np.array_equal(book.T, CR.update(rows, label, rows[[0, 5, 14]]))
    assert CR.build_codebook(rows.T, 15) is not None and CR.build_codebook(rows.T, 15).shape == (768, 15)


# ---------------------------------------------------------------------------------------------------- the C entry points
def test_argument_errors_are_reported_without_a_gpu():
    L = nat.lib()
    assert L.alive_codebook_update(None, 10, 768, None, None, 2, None, None, None) == -1
    assert b"null" in L.alive_last_error()
    assert L.alive_codebook_update(16, 10, 512, 16, 16, 2, 16, 16, None) == -1 and b"feature dim" in L.alive_last_error()
    assert L.alive_codebook_update(16, 10, 768, 16, 16, 0, 16, 16, None) == -1 and b"C=0" in L.alive_last_error()      # C < 1
    assert L.alive_codebook_update(16, 10, 768, 16, 16, 11, 16, 16, None) == -1 and b"C=11" in L.alive_last_error()    # C > M
    assert L.alive_codebook_update(16, 1 << 31, 768, 16, 16, 4, 16, 16, None) == -1 and b"M=2147483648" in L.alive_last_error()
    assert L.alive_codebook_update(16, 0, 768, 16, 16, 1, 16, 16, None) == -1 and b"M=0" in L.alive_last_error()
    assert L.alive_codebook_update(4, 10, 768, 16, 16, 2, 16, 16, None) == -1 and b"aligned" in L.alive_last_error()
    assert L.alive_codebook_stats(None, None, None, 10, None, None, None) == -1 and b"null" in L.alive_last_error()
    assert L.alive_codebook_stats(16, None, 16, 1 << 31, 16, 16, None) == -1 and b"M=2147483648" in L.alive_last_error()
    assert L.alive_codebook_stats(16, None, 16, 0, 16, 16, None) == -1 and b"M=0" in L.alive_last_error()


def test_workspace_query_is_positive_and_monotone_in_m():
    L = nat.lib()
    ws = lambda m, c: int(L.alive_codebook_workspace_bytes(m, c))      # noqa: E731
    for m, c in ((1000, 7), (70001, 300), (1000000, 65536)):
        sizes = [ws(mm, c) for mm in (m, m + 1, m + 511, m + 512, 2 * m, 16 * m)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
        # the plan (two offsets per list, one word per work item) plus at most 2 M / 512 + 1 slots of 768 doubles, each region padded
        assert sizes[0] <= 8 * (c + 1) + 4 * (c + m // 512) + (2 * (m // 512) + 1) * 768 * 8 + 4 * 256
    assert ws(1, 1) > 0
    for m, c in ((0, 1), (10, 0), (10, 11), (1 << 31, 5), (-1, 1)):
        assert ws(m, c) == 0


# ---------------------------------------------------------------------------------------------------- build_codebook's own checks
def test_build_codebook_refuses_bad_arguments_before_any_device_work():
    cpu = torch.zeros(768, 10)
    for bad in (0, -1, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="size"):
            CB.build_codebook(cpu, bad)
    with pytest.raises(ValueError, match="CPU tensor"):
        CB.build_codebook(cpu, 4)
    for shape in ((10, 768), (2, 768, 10), (768,)):
        with pytest.raises(ValueError, match=r"\[768, M\]"):
            CB.build_codebook(torch.zeros(*shape), 4)
    with pytest.raises(ValueError, match="iters"):
        CB.build_codebook(cpu, 4, iters=0)
    assert CB.check_init([3, 0, 9], 3, 10) == [3, 0, 9]
    for init, msg in (([0, 1], "3 integer row indices"), ([0, 1, 1], "twice"), ([0, 1, 10], "outside"), ([-1, 1, 2], "outside"),
                      ([0.5, 1, 2], "integer"), (5, "row indices")):
        with pytest.raises(ValueError, match=msg):
            CB.check_init(init, 3, 10)


# ---------------------------------------------------------------------------------------------------- the sessions file
def _load(tmp_path, sessions, **kw):
    p = tmp_path / "sessions.json"
    json.dump(sessions, open(p, "w"))
    return MSI.load_sessions(str(p), **kw)


def test_sessions_file_codebook_key(tmp_path):
    base = {"input": "a.wav", "lib": "l.pt"}
    ss = _load(tmp_path, [dict(base, codebook=1), dict(base, codebook=4096), dict(base, codebook=None), base])
    assert [s.get("codebook") for s in ss] == [1, 4096, None, None]
    assert "codebook" not in ss[2] and "codebook" not in ss[3]
    for bad in (0, -3, 2.5, "64", True, [64]):
        with pytest.raises(ValueError, match=r"session 1: \"codebook\" must be an integer >= 1 or null"):
            _load(tmp_path, [base, dict(base, codebook=bad)])
    # --codebook is the default of every session; a session's own key, null included, overrides it
    ss = _load(tmp_path, [base, dict(base, codebook=None), dict(base, codebook=32)], codebook=512)
    assert [s.get("codebook") for s in ss] == [512, None, 32]
    with pytest.raises(ValueError, match="--codebook"):
        _load(tmp_path, [base], codebook=0)


def test_the_size_is_part_of_the_voice_name(tmp_path):
    base = {"input": "a.wav", "target": "spk.wav", "lib": "l.pt"}
    a, b, c, d = _load(tmp_path, [dict(base, codebook=64), dict(base, codebook=128), base, dict(base, codebook=64)])
    names = [MSI.session_voice(s) for s in (a, b, c, d)]
    assert names[0] != names[1] and names[0] != names[2] and names[1] != names[2] and names[0] == names[3]
    assert names[2] == MSI.voice_name(c["target"], c["lib"]) == json.dumps([c["target"], c["lib"]])      # the name it always had
    blend = _load(tmp_path, [{"input": "a.wav", "codebook": 16, "blend": [{"lib": "/x/l.pt", "weight": 1}, {"lib": "/x/m.pt", "weight": 3}]}])[0]
    assert MSI.session_voice(blend) == [(MSI.voice_name(None, "/x/l.pt", 16), 1), (MSI.voice_name(None, "/x/m.pt", 16), 3)]


def test_a_file_without_the_key_parses_to_what_it_did(tmp_path):
    entries = [{"input": "a.wav", "lib": "l.pt"}, {"input": "b.wav", "target": "t.wav", "k": 2, "pitch": 3, "gate_db": -40}]
    ss = _load(tmp_path, entries)
    assert set(ss[0]) == set(MSI.SESSION_KEYS) and set(ss[1]) == set(MSI.SESSION_KEYS) | set(MSI.GATE_KEYS)
    base = str(tmp_path)
    assert ss[0] == dict(input=os.path.join(base, "a.wav"), target=None, lib=os.path.join(base, "l.pt"), output=None, pitch=0.0,
                         f0_rate=1.0, alpha=0.0, gain=0.0, input_gain=0.0, start=0, sr=None, world_pitch=False, blend=None, k=4,
                         auto_pitch=False, register_hz=None)
    assert MSI.build_parser().parse_args(["s.json"]).codebook is None
