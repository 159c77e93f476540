"""The host side of the WORLD pitch stage tests: the library's taps and plan (alive_world_f0_taps, alive_world_f0_layout: host arithmetic,
no GPU) against the restatement (tools/world_ref.py), the restatement's stage outputs against its own dio_rows, and the cases of
tests/world_cases.py against what they are there to reach: every interval count a stream can take, contours that are not blank, the
largest StoneMask window, and no StoneMask decision so close to a branch that the device test's 1e-6 on the f0 could hide one."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import world_cases as wc  # noqa: E402
from world_cases import W  # noqa: E402

CASES = wc.cases()


def lib():
    from module import _native as nat
    return nat.lib()


@pytest.mark.parametrize("cfg", wc.CONFIGS, ids=str)
def test_library_taps_are_the_restatements_bit_for_bit(cfg):
    fs, lo, hi, _ = cfg
    L = lib()
    n = L.alive_world_f0_taps_count(fs, lo, hi)
    lc, bl = W.taps(fs, lo, hi)
    want = np.concatenate([lc] + [w for _, w in bl])
    assert n == len(want)
    got = np.full(n + 8, np.nan)
    assert L.alive_world_f0_taps(fs, lo, hi, got.ctypes.data) == 0
    assert np.isnan(got[n:]).all()
    assert np.array_equal(got[:n].view(np.int64), want.view(np.int64))
    if cfg == wc.CONFIGS[2]:
        assert bl[0][0] == 256 and len(bl[0][1]) == 1024        # the lowest band fills the sweep's tile buffer exactly
    if fs == 16000:
        assert len(lc) == 641


@pytest.mark.parametrize("cfg", wc.CONFIGS, ids=str)
def test_layout_is_the_restatements_plan(cfg):
    fs, lo, hi, period = cfg
    L = lib()
    lc, bl = W.taps(fs, lo, hi)
    bnd = W.bands(lo, hi)
    for N, L8 in ((1, 1), (3, 1023), (4, 1024), (3, 2600), (4, 5000)):
        v = wc.layout(L, N, L8, cfg)
        F = W.n_frames(L8, fs, period)
        c = (len(lc) - 1) // 2
        assert (v["F"], v["nb"], v["c"], v["Ly"], v["yl_ld"]) == (F, len(bnd), c, L8 + 1, L8 + 1 + 2 * c)
        assert v["h"] == [h for h, _ in bl]
        assert np.array_equal(v["bound"].view(np.int64), np.array(bnd).view(np.int64))
        off = len(lc)
        for b, (h, w) in enumerate(bl):
            assert v["woff"][b] == off
            off += len(w)
        assert off == L.alive_world_f0_taps_count(fs, lo, hi)
        # the ten buffers: ascending, 256-aligned, not overlapping, inside the workspace
        nb = len(bnd)
        sizes = dict(mean=8 * N, yl=8 * N * v["yl_ld"], iv=8 * N * nb * 4 * F, ni=4 * N * nb * 4, best=8 * N * F, s1=8 * N * F,
                     s2=8 * N * F, s3=8 * N * F, pos=4 * N * F, neg=4 * N * F)
        end = 0
        for name in wc.OFFSETS:
            o = v["off"][name]
            assert o % 256 == 0 and o >= end, (name, o, end)
            end = o + sizes[name]
        assert v["off"]["mean"] == 0 and end <= v["total"] < end + 256 and v["total"] % 256 == 0
        assert v["total"] == L.alive_world_f0_workspace_bytes(N, L8, fs, lo, hi, period)


def test_refused_plans_are_refused():
    L = lib()
    for cfg in wc.REFUSED:
        assert L.alive_world_f0_workspace_bytes(3, 2600, *cfg) == 0, cfg
        assert wc.layout(L, 3, 2600, cfg) < 0, cfg
        assert L.alive_world_f0_taps_count(cfg[0], cfg[1], cfg[2]) < 0, cfg
    assert wc.layout(L, 0, 2600, wc.CONFIGS[0]) < 0 and wc.layout(L, 3, 0, wc.CONFIGS[0]) < 0
    assert W.matlab_round(16000 / (20.0 * 2 ** 0.5) / 2.0) == 283            # what refuses the first: 1132 taps
    # a short or missing output is refused, and nothing is written
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    assert L.alive_world_f0_layout(3, 2600, 8000, 20.0, 4096.0, 5.0, ctypes.cast(out, ctypes.c_void_p), 8) == -10
    assert list(out) == [-7] * 8
    assert L.alive_world_f0_layout(3, 2600, 8000, 20.0, 4096.0, 5.0, None, 64) == -10


def test_case_lengths_reach_what_they_are_for():
    for ci, cfg in enumerate(wc.CONFIGS[:wc.GRID]):
        fs, lo, _, period = cfg
        Ls = wc.lengths(cfg)
        vr, c = W.voice_range(period, lo), W.matlab_round(fs / 50.0)
        frames = {W.n_frames(L, fs, period) for L in Ls}
        assert {1, vr, vr + 1} <= frames and min(f for f in frames if f > 1) < vr
        assert {(L + 1 + 2 * c) % 256 for L in Ls} >= {255, 0, 1}
        assert {1023, 1024, 2047, 2048, 3071, 3072} <= {L + 1 for L in Ls} | set(Ls)        # Ly = L + 1 at and beside a tile
        assert max(Ls) <= wc.MAX_L
        kinds = set()
        for L in Ls:
            k = wc.case_kinds((ci, L))
            assert len(k) in (3, 4) and wc.case_rows((ci, L)).shape == (len(k), L)
            assert wc.case_rows((ci, L)).dtype == np.float32
            kinds |= set(k)
        assert kinds == set(wc.KINDS[fs])


@pytest.mark.parametrize("case", CASES, ids=wc.case_id)
def test_stages_agree_with_dio_rows_and_stonemask_has_margin(case):
    """dio_stages is what dio_rows returns (one copy of the arithmetic: the candidates are recombined here from the streams), and
    every voiced frame's StoneMask decisions keep a relative margin of 1e-5, ten times the bound the device test puts on the f0:
    a device value within that bound of the restatement's takes the same branches, so the bound hides no wrong branch"""
    cfg = wc.CONFIGS[case[0]]
    X = wc.case_rows(case).astype(np.float64)
    rows, t = wc.case_stages(case)
    f0, t2 = W.dio_rows(X, *cfg)
    assert np.array_equal(t, t2) and len(rows) == X.shape[0]
    F, nb, c = len(t), len(W.bands(cfg[1], cfg[2])), W.matlab_round(cfg[0] / 50.0)
    vr = W.voice_range(cfg[3], cfg[1])
    for r, row in enumerate(rows):
        assert np.array_equal(row["f0"], f0[r])
        assert row["yl"].shape == (X.shape[1] + 1 + 2 * c,) and row["ni"].shape == (nb, 4) and row["cand"].shape == (nb, F)
        for b in range(nb):
            for st in range(4):
                assert (row["iv"][b][st] is None) == (row["ni"][b, st] < 2)
            if row["ni"][b].min() > 2:
                iv = row["iv"][b]
                cand = (((iv[0] + iv[1]) + iv[2]) + iv[3]) / 4.0
                assert np.all((row["cand"][b] == cand) | (row["cand"][b] == 0))
            else:
                assert not row["cand"][b].any()
        assert (row["s1"] is None) == (row["s2"] is None) == (F <= vr)
        if F <= vr:
            assert not row["f0"].any()
        for f in np.nonzero(row["f0"] > 0)[0]:
            m = W.stonemask_margin(X[r], cfg[0], t[f], row["f0"][f])
            assert m >= 1e-5, (r, f, row["f0"][f], m)


def test_cases_cover_the_sweeps_edges():
    """over all cases: streams with 0, 1, 2, 3 and more intervals in every configuration; bands that lose everywhere but hold
    values; voiced contours in every configuration, with frames on both sides of StoneMask's gates; its window at 1201 samples"""
    for ci, cfg in enumerate(wc.CONFIGS[:wc.GRID]):
        counts, voiced, gated, losing, window = set(), 0, 0, 0, 0
        for case in CASES:
            if case[0] != ci:
                continue
            rows, t = wc.case_stages(case)
            for row in rows:
                counts |= set(np.minimum(row["ni"], 4).ravel().tolist())
                v = row["f0"] > 0
                ok = v & ~((row["f0"] <= 40.0) | (row["f0"] > cfg[0] / 12.0))
                voiced += int(ok.sum())
                gated += int((v & ~ok).sum())
                if ok.any():
                    window = max(window, 2 * W.matlab_round(1.5 / row["f0"][ok].min() * cfg[0]) + 1)
                losing += sum(1 for b in range(len(row["cand"])) if row["ni"][b].min() >= 2 and not row["cand"][b].any())
        assert counts == {0, 1, 2, 3, 4}, (cfg, counts)
        assert voiced >= 100 and losing > 0, (cfg, voiced, losing)
        if cfg[1] < 40.0:
            assert gated > 0, cfg
        if cfg == wc.CONFIGS[2]:
            assert window == 1201


def test_knot_case_puts_a_frame_on_an_interval_location_at_a_tile_end():
    """the extra configuration's reason to exist, on the restatement alone: the frame's time equals the interval's location
    exactly, the interval is the newest when the sweep's first tile ends, more follow, and extrapolating from the segment before
    it would round differently from the interval's own value, which is what interp1 gives at its knot"""
    case = (wc.CONFIGS.index(wc.KNOT), wc.KNOT_L)
    fs, lo, hi, period = wc.KNOT
    at = wc.KNOT_AT
    assert at["stream"] == 0
    X = wc.case_rows(case).astype(np.float64)
    rows, t = wc.case_stages(case)
    _, yl = W.lowcut_signals(X, fs, lo, hi)
    s = W.band_signals(yl, X.shape[1], fs, lo, hi)[at["band"]][at["row"]]
    e = np.nonzero((s[:-1] > 0.0) & (s[1:] <= 0.0))[0] + 1
    fine = e - s[e - 1] / (s[e] - s[e - 1])
    loc, val = (fine[:-1] + fine[1:]) / 2.0 / fs, fs / (fine[1:] - fine[:-1])
    q, f = at["interval"], at["frame"]
    assert t[f] == f * period / 1000.0 == loc[q]
    assert e[q + 1] < 1024 <= e[q + 2] and len(loc) > q + 1 and q >= 1
    assert val[q - 1] + 1.0 * (val[q] - val[q - 1]) != val[q]
    assert rows[at["row"]]["ni"][at["band"], 0] == len(loc)
    assert rows[at["row"]]["iv"][at["band"]][0][f] == val[q]
