"""The NumPy codec reference of the kNN stage tests (tests/knn_codes.py) against the formats' definitions, and the stage tests' shapes
against the search plans: no GPU needed (alive_debug_knn_stage_view is host arithmetic on ws_layout / make_plan)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_codes as kc  # noqa: E402


def _e2m3_value(code):
    """a code's value from the format's definition, one code at a time"""
    s, e, m = (code >> 5) & 1, (code >> 3) & 3, code & 7
    mag = m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1)
    return -mag if s else mag


def test_e2m3_grid_and_round_trip_of_all_codes():
    codes = np.arange(64, dtype=np.uint8)
    vals = kc.e2m3_decode(codes)
    assert [float(v) for v in vals] == [_e2m3_value(int(c)) for c in codes]
    mags = vals[:32]
    # steps of 1/8 up to 2, 1/4 up to 4, 1/2 up to 7.5
    steps = np.diff(mags)
    assert np.all(steps[mags[:-1] < 2.0] == 0.125) and np.all(steps[(mags[:-1] >= 2.0) & (mags[:-1] < 4.0)] == 0.25)
    assert np.all(steps[mags[:-1] >= 4.0] == 0.5) and mags[-1] == 7.5 == kc.E2M3_MAX
    back = kc.e2m3_encode(vals)
    assert np.array_equal(back, codes)                                     # -0.0 (code 32) keeps its sign bit
    assert kc.e2m3_encode(np.array([0.0]))[0] == 0 and kc.e2m3_encode(np.array([-0.0]))[0] == 32
    assert np.signbit(kc.e2m3_decode(np.array([32]))[0]) and kc.e2m3_decode(np.array([32]))[0] == 0.0


def test_e2m3_midpoints_round_to_the_even_code():
    mags = kc.E2M3_MAG
    for c in range(31):
        mid = (mags[c] + mags[c + 1]) / 2.0
        even = c if c % 2 == 0 else c + 1
        for sign, bit in ((1.0, 0), (-1.0, 32)):
            assert kc.e2m3_encode(np.array([sign * mid]))[0] == (even | bit), (c, sign)
            # one float32 step to either side of the midpoint goes to the nearer neighbour
            below, above = np.nextafter(np.float32(mid), np.float32(0)), np.nextafter(np.float32(mid), np.float32(8))
            assert kc.e2m3_encode(np.array([sign * float(below)]))[0] == (c | bit)
            assert kc.e2m3_encode(np.array([sign * float(above)]))[0] == ((c + 1) | bit)


def test_e2m3_saturates_at_7_5():
    for y in (7.5, 7.500001, 7.6, 7.75, 7.76, 8.0, 31.9, 1.0e6, float("inf")):
        assert kc.e2m3_encode(np.array([y]))[0] == 31 and kc.e2m3_encode(np.array([-y]))[0] == 63, y
    assert kc.e2m3_encode(np.array([7.25]))[0] == 30            # the midpoint below the top goes to the even code 30 = 7.0
    assert kc.e2m3_encode(np.array([7.2500005]))[0] == 31


def test_slot_image_round_trips_random_codes():
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 64, size=(7, 24, 32), dtype=np.uint8)
    img = kc.slots_pack(codes)
    assert img.shape == (7, 24, 32) and img.dtype == np.uint8
    assert not img[..., 24:].any()
    back, tail = kc.slots_unpack(img)
    assert np.array_equal(back, codes) and not tail.any()
    # the bit stream, spelled out for one slot: code j sits at bits 6 j .. 6 j + 5 of the little-endian 192-bit number
    one = codes[3, 5]
    n = sum(int(c) << (6 * j) for j, c in enumerate(one))
    assert bytes(img[3, 5, :24]) == n.to_bytes(24, "little")
    # and the row forms used on whole images
    vals = kc.e2m3_decode(codes).reshape(7, 768)
    assert np.array_equal(kc.fp6_image(vals), img.reshape(7, 768))
    assert np.array_equal(kc.fp6_image_decode(img.reshape(7, 768)), vals)


def test_e4m3_decode_and_encode_agree_with_torch():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    got = kc.e4m3_decode(codes)
    nan = (codes & 127) == 127
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(got[~nan], want[~nan]) and np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan]))
    assert got[126] == 448.0 and got[1] == 2.0 ** -9
    # encode: every code's value comes back; ties go to the even code; a dense sweep agrees with torch's round-to-nearest-even cast
    assert np.array_equal(kc.e4m3_encode(got[~nan]), codes[~nan])
    mags = kc.E4M3_MAG
    mids = (mags[:-1] + mags[1:]) / 2.0
    assert np.array_equal(kc.e4m3_encode(mids), np.array([c if c % 2 == 0 else c + 1 for c in range(126)], np.uint8))
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.standard_normal(20000) * 10.0, rng.standard_normal(20000) * 0.01, mids, -mids]).astype(np.float32)
    t = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(kc.e4m3_encode(x), t)


def test_bf16_decode():
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1)).bfloat16()
    assert np.array_equal(kc.bf16_decode(x.view(torch.int16).numpy().view(np.uint16)), x.float().numpy())


# ---- the stage tests' shapes against the plans ---------------------------------------------------------------------------------

def _views(shapes, sub):
    from module import _native as nat
    L = nat.lib()
    return [(n, t, m, kc.stage_view(L, n * t, m, kc.K, sub)) for n, t, m in shapes]


def test_stage_view_is_consistent():
    for n, t, m, v in _views(kc.SHAPES, False) + _views(kc.SUB_SHAPES, True):
        Tt = n * t
        assert (v["KP"], v["KP8"], v["FT"], v["FT6"], v["LT"]) == (16, 32, 256, 384, 32)
        m_pad = (m + 127) // 128 * 128
        for name, ft in (("p16", v["FT"]), ("p8", v["FT"]), ("p6", v["FT6"])):
            p = v[name]
            assert p["Tt_pad"] == (Tt + ft - 1) // ft * ft and p["tiles_total"] * v["LT"] == m_pad
            assert p["P"] * p["tiles_per_split"] >= p["tiles_total"] and p["P"] >= 1
        offs = [v[f] for f in ("s_bf16", "s_f8", "cv", "ci", "clip6")]
        assert all(o > 0 and o % 256 == 0 and o < v["bytes"] for o in offs) and len(set(offs)) == 5
    assert all(v["sub_f6"] == -1 and v["sub_g"] == -1 for _, _, _, v in _views(kc.SHAPES, False))
    assert all(0 < v["sub_f6"] < v["sub_g"] < v["bytes"] for _, _, _, v in _views(kc.SUB_SHAPES, True))
    from module import _native as nat
    assert nat.lib().alive_debug_knn_stage_view(0, 10, 4, 0, None, 25) == -1


@pytest.mark.parametrize("stage", ["fp6", "fp8", "fp6-subspace"])
def test_shapes_reach_every_edge_of_the_split_loop(stage):
    """The stage tests read the plans from the view instead of hard-coding them; this is the guard that a change of make_plan cannot thin
    them out silently: for each block-scaled stage the shapes must include more than one library split, a split with an odd and one with
    an even number of tiles (the last tile's accumulators end in the other register set), and a split with no tiles at all."""
    sub = stage == "fp6-subspace"
    plan = "p8" if stage == "fp8" else "p6"
    counts = [kc.split_tiles(v[plan]) for _, _, _, v in _views(kc.SUB_SHAPES if sub else kc.SHAPES, sub)]
    assert any(len(c) > 1 for c in counts), counts
    flat = [x for c in counts for x in c]
    assert any(x % 2 == 1 for x in flat), counts
    assert any(x > 0 and x % 2 == 0 for x in flat), counts
    assert any(x == 0 for x in flat), counts
    # frame blocks: a batch that ends inside a block and one that fills its block exactly
    ft = 256 if stage == "fp8" else 384
    tts = [n * t for n, t, _ in (kc.SUB_SHAPES if sub else kc.SHAPES)]
    assert any(tt % ft for tt in tts)
    if not sub:
        assert any(tt > ft for tt in tts) and 384 in tts and 385 in tts
