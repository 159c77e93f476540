"""CPU twin of tests/test_gpu_glue_exact.py: the cases of tests/glue_cases.py are what they claim to be -- the sums are exact in fp32 in
any order, the expected bits are those of a float64 reference, the special columns sit where the kernels' merges can get them wrong.
No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_cases as G  # noqa: E402

F32 = np.float32


# ---- A ----
def test_norm_shapes_cover_the_matrix():
    for ts, small in ((G.NORM_T_SMALL, True), (G.NORM_T_TILED, False)):
        side = [(c, t) for c, t in G.NORM_SHAPES if (t <= 32) == small]
        assert {c for c, _ in side} == set(G.NORM_C)                            # every C on this side of the switch
        for t in ts:
            assert len({c for c, tt in side if tt == t}) == 2                   # every T at two values of C
    assert {c for c, _ in G.PLANE_SHAPES} == {64, 256, 512}


def _f32_sum(a, order):
    """sequential fp32 sum over the channels of a [n][c][t], taken in `order`"""
    return np.cumsum(a[:, order].astype(F32), axis=1, dtype=F32)[:, -1]


@pytest.mark.parametrize("c,t", G.NORM_SHAPES + G.PLANE_SHAPES)
def test_norm_columns_are_exact(c, t):
    case = G.norm_case(c, t)
    x, w, b, y = case["x"], case["w"], case["b"], case["y"]
    assert np.abs(w).max() <= 3 and np.abs(b).max() <= 4 and np.abs(np.delete(x, case["cb"], axis=1)).max() <= 8
    assert (w[case["cb"]] == (0, 0, 0, 1, 0, 0, 0)).all() and np.abs(x[:, case["cb"]]).max() <= 8 + c // 2 + 1
    assert (np.diff(np.delete(w, case["cb"], axis=0), axis=1) != 0).all(), "neighbouring taps differ"
    # y is the float64 depthwise conv
    ref = F.conv1d(torch.from_numpy(x).double(), torch.from_numpy(w).double().view(c, 1, 7), torch.from_numpy(b).double(), padding=3, groups=c)
    assert np.array_equal(ref.numpy(), y.astype(np.float64))
    # integer statistics inside the fp32 budget: every partial sum of |y|, and of the squares, is below 2^24
    s = y.sum(1)
    assert not (s % c).any(), "column sums divisible by C"
    mean, ss = G.norm_stats(y)
    assert np.abs(y).sum(1).max() < G.BUDGET and ss.max() < G.BUDGET and np.abs(y).max() < 2 ** 11
    print(f"C {c} T {t}: max |y| {np.abs(y).max()}, max sum |y| {np.abs(y).sum(1).max()}, max ss {ss.max()}")
    # ... so fp32 sums in two channel orders give the integers, and the expected bits do not depend on the order
    fwd, perm = np.arange(c), np.random.default_rng(c * 1000 + t).permutation(c)
    d = y - mean
    for order in (fwd, perm, fwd[::-1]):
        assert np.array_equal(_f32_sum(y, order).astype(np.int64), s)
        assert np.array_equal(_f32_sum((d * d), order).astype(np.int64), ss[:, 0])
    # the expected bits against float64, one rounding at a time
    for eps in G.NORM_EPS:
        for adaptive in (False, True):
            want = G.norm_expected(case, eps, adaptive)
            var = (ss.astype(np.float64) / (c - 1)).astype(F32)                  # fp32(ss) is ss: one rounding
            sigma = (np.sqrt(var.astype(np.float64)).astype(F32).astype(np.float64) + np.float64(F32(eps))).astype(F32)
            v = (d.astype(np.float64) / sigma.astype(np.float64)).astype(F32)
            if adaptive:
                g, o = case["cond"][:, 3:3 + c], case["cond"][:, c + 5:2 * c + 5]
            else:
                g, o = case["gain"][None, :, None], case["offset"][None, :, None]
            assert (np.abs(g) == 2.0 ** np.round(np.log2(np.abs(g)))).all(), "gains are signed powers of two"
            ref64 = (v.astype(np.float64) * g.astype(np.float64) + o.astype(np.float64)).astype(F32)     # v g exact: one rounding
            assert np.array_equal(want.view(np.uint32), ref64.view(np.uint32))
            assert np.isfinite(want).all()
            # near the true value: the construction did not drift from the operation it stands for
            true = d / (np.sqrt(ss / (c - 1)) + eps) * g.astype(np.float64) + o.astype(np.float64)
            assert np.abs(want - true).max() <= 4e-6 * max(1.0, np.abs(true).max())
            if (c, t) in G.PLANE_SHAPES:
                assert bool(G.bf16_split3_lossless(want).all()), "a three-plane bf16 split of every expected element is lossless"
    assert case["rows"] > 2 * c and case["scale_row"] > 0 and case["shift_row"] > 0


# ---- B ----
@pytest.mark.parametrize("c", G.ARGMAX_C)
def test_argmax_columns(c):
    for t in G.ARGMAX_T:
        x, want, pats = G.argmax_case(c, t)
        n = x.shape[0]
        assert n * t >= len(pats), "every pattern occurs at this T"
        for q in range(n * t):
            col = x[q // t, :, q % t]
            assert want[q // t, 0, q % t].item() == G.first_max(col.tolist()), pats[q % len(pats)][0]
            name, fill, plants = pats[q % len(pats)]
            if fill is None:                                                     # the background is distinct values inside (-1, 1)
                bg = np.delete(col.numpy(), [ch for ch, _ in plants])
                assert len(set(bg.tolist())) == len(bg) and (np.abs(bg) < 1).all()
    names = [p[0] for p in G.argmax_patterns(c)]
    assert len(set(names)) == len(names)
    if c >= 301:
        assert {"tie 8 1", "NaNs 8 1", "tie 300 9", "NaNs 300 9", "NaNs 8 4", "NaN below +inf", "all -inf"} <= set(names)


def test_argmax_pairs_sit_where_the_merges_are():
    for hi, lo in ((8, 1), (300, 9)):
        assert lo % 4 > hi % 4, "tiled kernel: the lower channel belongs to a wave that is merged later"
        assert lo % 256 != hi % 256, "per-frame kernel: two threads"
    half = lambda row: (row % 8) // 4
    assert half(8) == 0 and half(4) == 1, "GEMM epilogue: row 8 in the receiving half-wave, row 4 in the other"
    assert 70 // 64 != 5 // 64, "two 64-row blocks"


@pytest.mark.parametrize("co", G.GEMM_ARGMAX_CO)
def test_gemm_argmax_cases(co):
    for name, w, x, b, want, y in G.gemm_argmax_cases(co):
        assert bool(G.bf16_split3_lossless(w).all()) and bool(G.bf16_split3_lossless(x).all())
        assert (w.abs().sum(1).max() * x.abs().max()).item() < 300 < G.BIG
        for col in range(x.shape[2]):
            assert want[0, 0, col].item() == G.first_max(y[:, col].tolist()), name
        _, fill, plants = next(p for p in G.argmax_patterns(co) if p[0] == name)
        for ch, v in plants:                                                     # the product is exactly the planted value
            assert all((yy != yy) if v != v else yy == v for yy in y[ch].tolist())


# ---- C ----
@pytest.mark.parametrize("lw", G.SOURCE_IN_LW)
def test_source_in_operands_are_exact(lw):
    c = G.source_in_case(lw)
    assert c["units0"] < 2 ** 12 and c["units"] < G.BUDGET, (c["units0"], c["units"])
    assert torch.equal(c["x0"] * 2.0 ** 7, (c["x0"] * 2.0 ** 7).round()) and torch.equal(c["ref"] * 2.0 ** 10, (c["ref"] * 2.0 ** 10).round())
    assert torch.equal(c["ref"].float().double(), c["ref"]) and c["ref"].shape == (G.EDGE_N, 16, lw // 2)
    assert not torch.equal(c["src"][0], c["src"][1]) or lw < 4


@pytest.mark.parametrize("lw", G.SOURCE_OUT_LW)
def test_source_out_operands_are_exact(lw):
    c = G.source_out_case(lw)
    assert c["units"] < G.BUDGET
    assert torch.equal(c["ref"] * 2.0 ** 9, (c["ref"] * 2.0 ** 9).round()) and torch.equal(c["ref"].float().double(), c["ref"])
    assert not torch.equal(c["h"][0], c["h"][1])


# ---- D ----
@pytest.mark.parametrize("orig,new", G.RESAMPLE_PAIRS)
def test_resample_geometry(orig, new):
    width, taps = G.resample_width(orig, new), G.resample_taps(orig, new)
    assert width == int(np.ceil(6 * orig / (min(orig, new) * 0.99))) and taps == 2 * width + orig
    c = G.impulse_case(orig, new)
    assert (new * c["L"]) % orig != 0 and c["full"] == -(-new * c["L"] // orig)
    assert c["pos"][0][0] == 1 and c["pos"][1][0] == 0 and c["pos"][0][-1] == c["L"] - 1 and c["pos"][1][-1] == c["L"] - 2
    # the impulse response of the polyphase sum on a float64 bank: the index map picks exactly the entries
    bank = G.resample_bank64(orig, new)
    x = c["x"].astype(np.float64) * 2.0
    xpad = np.zeros((2, (c["full"] // new + 2) * orig + taps))
    xpad[:, width:width + c["L"]] = x
    for lout in c["louts"]:
        assert 0 < lout <= c["full"]
        idx = c["idx"](lout)
        for o in range(lout):
            m, p = divmod(o, new)
            y = xpad[:, m * orig:m * orig + taps] @ bank[p]
            want = np.where(idx[:, o] >= 0, bank.reshape(-1)[np.maximum(idx[:, o], 0)], 0.0)
            assert np.array_equal(y, want), (lout, o)
        for b in range(2):                                    # an impulse shows on either side of the block edge, and at both row ends
            assert idx[b, c["edge"] - 1] >= 0 and idx[b, c["edge"]] >= 0 and idx[b, 0] >= 0 and idx[b, lout - 1] >= 0
    # the last output sample's taps reach past the end of the row
    m_last = (c["full"] - 1) // new
    assert m_last * orig - width + taps - 1 >= c["L"]


def test_resample_banks_and_where_they_live():
    assert [G.bank_is_lds_staged(o, n) for o, n in G.RESAMPLE_PAIRS] == [True, True, True, False, False]
    for orig, new in G.RESAMPLE_PAIRS:
        b64 = G.resample_bank64(orig, new)
        assert b64.shape == (new, G.resample_taps(orig, new)) and np.isfinite(b64).all()
        share = G.bank_sensitive(b64).mean()
        print(f"{orig} -> {new}: {b64.size} taps, sensitive share {share:.2e}")
        assert share < 1e-4
        # a low-pass of unit DC gain: every phase sums to 1 within the window's leakage
        assert np.abs(b64.sum(1) - 1.0).max() < 0.02


@pytest.mark.parametrize("orig,new,length", G.DENSE_PAIRS)
def test_dense_resample_case_is_exact(orig, new, length):
    c = G.dense_case(orig, new, length)
    assert c["units"] < G.BUDGET and c["x"][1, 0] != 0
    assert np.array_equal(c["y"] * 1024.0, np.round(c["y"] * 1024.0)) and np.array_equal(c["y"].astype(F32).astype(np.float64), c["y"])
    assert (new * length) % orig != 0


# ---- E ----
@pytest.mark.parametrize("t", G.PITCH_T)
def test_pitch_rows_are_exact(t):
    for kind in G.PITCH_KINDS:
        j = G.pitch_row(kind, t)
        voiced = j != -99
        if kind == "none":
            assert not voiced.any()
        elif kind == "one":
            assert voiced.sum() == 1
        else:
            assert voiced.any() and j[voiced].mean() == -1 and ((j[voiced] + 1) % 2 == 0).all()
            if kind == "last stride":
                assert not voiced[:(t - 1) // 256 * 256].any()
            elif t > 1:
                assert 0 < voiced.sum() < t, "the count of voiced frames is not T"
        for mode in (0, 1):
            for params in G.PITCH_PARAMS:
                f0, y32, y64 = G.pitch_case(kind, t, mode, params)
                assert np.array_equal(y32.astype(np.float64), y64) and np.isfinite(y32).all()
                assert set(np.unique(f0)) <= {0.0, 55.0, 110.0, 220.0, 440.0, 880.0, 1760.0}
                assert ((y32 == 0) == ~voiced).all()
                # the reference's arithmetic in float64 on the same row
                with np.errstate(divide="ignore", invalid="ignore"):
                    if mode == 0:
                        p = 12 * np.log2(f0.astype(np.float64) / 440) - 9
                        mean = p[np.isfinite(p)].mean() if voiced.any() else np.nan
                        out = 440 * 2 ** ((mean + (p - mean) * params[2] + params[1] + 9) / 12)
                        out = np.where(np.isfinite(out), out, 0.0) * params[0]
                    else:
                        p = 12 * np.log2(f0.astype(np.float64) * params[0] / 440) - 9 + params[1]
                        out = 440 * 2 ** ((p + 9) / 12)
                        out = np.where(np.isfinite(out), out, 0.0)
                assert np.array_equal(out, y64), (kind, mode, params)


# ---- F ----
@pytest.mark.parametrize("c,spf", G.FILM_SHAPES)
def test_film_range_columns(c, spf):
    for lo, hi in G.FILM_RANGES:
        ok = G.film_range_columns(spf, (lo, hi))
        assert ok.shape == ((hi - lo) * spf,) and ok.sum() == (hi - lo - 1) * spf, "all but the first and the last half frame"
        assert not ok[:spf // 2].any() and not ok[-(spf // 2):].any() and ok[spf // 2:-(spf // 2)].all()
    assert G.film_range_columns(spf, G.FILM_RANGES[1]).mean() >= 0.9
    # lerp_frames against F.interpolate's coordinates: a ramp over the frames comes back as i0 + w1
    ramp = torch.arange(G.FILM_FRAMES, dtype=torch.float32).view(1, 1, -1)
    up = F.interpolate(ramp, size=G.FILM_FRAMES * spf, mode="linear", align_corners=False)[0, 0]
    for t in range(G.FILM_FRAMES * spf):
        i0, i1 = G.lerp_frames(t, F32(G.FILM_FRAMES) / F32(G.FILM_FRAMES * spf), G.FILM_FRAMES)
        assert i0 <= up[t].item() <= i1 + 1e-6 and i1 - i0 in (0, 1)
