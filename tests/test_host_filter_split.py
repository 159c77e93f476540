"""Host twin of tests/test_gpu_filter_split.py: the restatement of the fused split-bf16 FilterBlocks (tools/filter_split_ref.py; the kernels
are csrc/filter_small.hip and csrc/filter_mid.hip) is pinned to the oracle, its launch plans are pinned to the sources' constants, the null
band behind the GPU file's bars is measured, and the bars are shown to catch the defects these kernels could have.

The statistic: the error against the exact float64 block as rms per column (pooled over windows and channels), rms per channel (pooled
over windows and columns), total rms and largest single error.  Two emulations of the kernels' operand splits with different last-bit
behaviour in their epilogues give the same figures within the null band; a defect confined to a few columns or channels does not.
"""
import os
import re
import sys
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as F

import alive_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import filter_split_ref as R                                         # noqa: E402

SEEDS = (0, 1, 2, 3, 4)
GLOBAL_BOUND = 4e-5                            # test_fused_filter_block_small's check


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)).item()


# ---- agreement -----------------------------------------------------------------------------------------------------------
def _double_case(c, l, lf, n):
    sd, fw = R.block_weights(c)
    x, cnd, skip = R.inputs(c, l, lf, n)
    sd64 = {k: v.double() for k, v in sd.items()}
    film = F.conv1d(cnd.double(), fw[0].double(), fw[1].double()) + fw[2].double().view(1, -1, 1)
    return sd64, x.double(), cnd.double(), skip.double(), film


@pytest.mark.parametrize("case", R.ACCURACY, ids=lambda s: s.name)
def test_the_exact_flavour_is_the_oracles_filter_block(case):
    """rounding=False against O.filter_block + skip on float64 tensors, two windows of every accuracy case: the input conv, the FiLM rows at
    their offset in a larger table, ATen's float64 interpolation, the reflected causal convs at dilations 1, 1, 2, 2, 4, 4, the residual
    behind every second one"""
    sd64, x, cnd, skip, film = _double_case(case.C, case.l, case.lf, 2)
    ref = O.filter_block(sd64, "n", x, cnd) + skip
    out = R.filter_block_split(x, film, R.PAD_ROWS, sd64, "n", skip=skip, rounding=False)
    assert out.dtype == torch.float64 and out.shape == ref.shape
    assert (out - ref).abs().max().item() <= 1e-12 * ref.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("rc", R.RANGES, ids=lambda r: f"{r.C}-f{r.f0}")
def test_the_exact_flavour_in_a_frame_range_is_the_whole_signals_columns(rc):
    """a frame range from a table that holds its frames only (t0 / f0 / frames): inside the margins the samples are the oracle's on the
    whole signal, the first 16 columns are the window's own (its reflected start)"""
    up, lf = rc.up, rc.frames
    sd64, x, cnd, skip, film = _double_case(rc.C, up * lf, lf, 1)
    whole = O.filter_block(sd64, "n", x, cnd) + skip
    cut = slice(up * rc.f0, up * (rc.f0 + rc.nf))
    part = R.filter_block_split(x[:, :, cut], film[:, :, rc.f0:rc.f0 + rc.nf], R.PAD_ROWS, sd64, "n", skip=skip[:, :, cut], t0=up * rc.f0,
                                f0=rc.f0, frames=lf, rounding=False)
    lo, hi = rc.margins
    scale = whole.pow(2).mean().sqrt().item()
    assert (part[:, :, lo:hi] - whole[:, :, up * rc.f0 + lo:up * rc.f0 + hi]).abs().max().item() <= 1e-12 * scale
    assert (part[:, :, :16] - whole[:, :, up * rc.f0:up * rc.f0 + 16]).abs().max().item() > 1e-3 * scale


@lru_cache(maxsize=None)
def _flavours(c, l, lf, n, seed):
    sd, fw = R.block_weights(c, seed)
    x, cnd, skip = R.inputs(c, l, lf, n, seed)
    film = R.film_table(cnd, fw)
    return (R.filter_block_split(x, film, R.PAD_ROWS, sd, "n", skip=skip, rounding=False),
            R.filter_block_split(x, film, R.PAD_ROWS, sd, "n", skip=skip, flavour="f32"),
            R.filter_block_split(x, film, R.PAD_ROWS, sd, "n", skip=skip, flavour="f64"))


def _both_ways(r):
    r = torch.as_tensor(r, dtype=torch.float64).reshape(-1)
    return min(r.min().item(), (1.0 / r).min().item()), max(r.max().item(), (1.0 / r).max().item())


def test_the_null_band_of_two_emulations_lies_inside_the_recorded_one():
    """every accuracy case of the GPU file x five seeds.  Agreement: both flavours sit at the split product's distance from the exact
    block (2^-17 per product: 4 .. 9e-6 of the output here), well inside the global bound, and differ from each other by fp32
    rounding only (less than from the exact block).  The null band: the ratio of the flavours' column profiles, channel profiles, total
    and largest errors, either over the other; the recorded constants (tools/filter_split_ref.py::NULL_BAND, rounded outwards to two
    decimals) still contain the extremes, and BARS is that band widened by 1.25."""
    band = {}
    for case in R.ACCURACY:
        case.plan()
        for seed in SEEDS:
            ex, a, b = _flavours(case.C, case.l, case.lf, case.n, seed)
            ea, eb, ab = relerr(a, ex), relerr(b, ex), relerr(a, b)
            assert 2e-6 < ea < 0.5 * GLOBAL_BOUND and 2e-6 < eb < 0.5 * GLOBAL_BOUND, (case.name, seed, ea, eb)
            assert 0 < ab < min(ea, eb), (case.name, seed, ab, ea, eb)
            d = band.setdefault(case.key, {s: [9.0, 0.0] for s in ("column", "channel", "total", "peak")})
            for stat, r in R.profile_ratios(a, b, ex).items():
                lo, hi = _both_ways(r)
                d[stat] = [min(d[stat][0], lo), max(d[stat][1], hi)]
            _flavours.cache_clear()
    print("measured null band:", {k: {s: (round(v[0], 4), round(v[1], 4)) for s, v in d.items()} for k, d in band.items()})
    assert set(band) == set(R.NULL_BAND)
    for key, d in band.items():
        for stat, (lo, hi) in d.items():
            rlo, rhi = R.NULL_BAND[key][stat]
            assert rlo <= lo and hi <= rhi, (key, stat, (lo, hi), (rlo, rhi))
            assert rlo >= lo - 0.02 and rhi <= hi + 0.02, (key, stat, (lo, hi), "the recorded band is wider than the measured one")
            blo, bhi = R.BARS[key][stat]
            assert blo == rlo / 1.25 and bhi == rhi * 1.25 and blo < 1.0 < bhi


# ---- the plans against the sources -----------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(ROOT, "alive-vc_amd", "csrc", name)) as f:
        return f.read()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def test_small_plan_restates_filter_small_hip():
    s = _src("filter_small.hip")
    assert int(_one(r"constexpr int HALO = (\d+);", s)) == R.HALO
    assert int(_one(r"constexpr int NFP = (\d+);", s)) == R.SMALL_NFP
    assert int(_one(r"constexpr int PLANE_BATCH = (\d+);", s)) == R.SMALL_PLANES[2]
    assert _one(r"static constexpr int ROWB = ([^;]+);", s) == "2 * C" and _one(r"static constexpr int BL = ([^;]+);", s) == "PLANE / ROWB"
    assert _one(r"static constexpr int HL = ([^;]+);", s) == "TAIL == TAIL_WAVE ? HALO + 8 : HALO" and _one(r"static constexpr int TT = ([^;]+);", s) == "BL - HL"
    assert int(_one(r"const bool tiny = pl_env \? pl_env < \d+ : big_tiles <= (\d+);", s)) == R.SMALL_TINY_TILES
    assert int(_one(r"const bool tiny = pl_env \? pl_env < (\d+) :", s)) == R.SMALL_PLANES[1]
    assert _one(r"const int big_tiles = ([^;]+);", s) == "cdiv(L, (C == 8 ? Cfg<8>::TT : Cfg<16>::TT)) * N"
    assert _one(r"if \(!tiny && \(([^)]+)\)\)", s) == "pl_env == 16384 || pl_env == 0"
    assert set(re.findall(r"launch_small<(?:8|16), (\w+)>\(", s)) == {"8192", "16384", "PLANE_BATCH"}
    assert int(_one(r"const bool small = \(int64_t\)tiles \* N <= (\d+);", s)) == R.FIRST_ONLY_TILES
    assert _one(r"ALIVE_CHECK_ARG\(\(double\)([^,]+) <= NFP,", s) == "K::BL * film_ld / L + 3.0"
    # the tiles: (BL, TT) per <C, PL>
    assert [R.small_tile(16, pl) for pl in R.SMALL_PLANES] == [(256, 200), (512, 456), (1024, 968)]
    assert [R.small_tile(8, pl) for pl in R.SMALL_PLANES] == [(512, 456), (1024, 968), (2048, 1992)]
    # hand-worked: the streaming step, the bench window, the env switch that reaches <C, false, 8192>
    p = R.small_plan(16, 1, 1600)
    assert (p.PL, p.tiles, p.all_first) == (8192, 8, True)
    p = R.small_plan(8, 64, 144000)
    assert (p.PL, p.TT, p.tiles, p.all_first) == (16384, 968, 149, False)
    assert R.small_plan(16, 16, 968).PL == 8192 and R.small_plan(16, 16, 972).PL == 16384 and R.small_plan(16, 17, 968).PL == 16384
    p = R.small_plan(16, 5, 10400, plane_env=8192)
    assert (p.PL, p.tiles * p.N, p.forms) == (8192, 260, ((16, True, 8192), (16, False, 8192)))
    p = R.small_plan(8, 5, 23720, plane_env=8192)
    assert (p.PL, p.tiles, p.all_first) == (8192, 53, False)
    assert R.small_plan(8, 5, 23720, plane_env=32768).PL == 32768 and R.small_plan(8, 1, 3200, plane_env=32768).forms == ((8, True, 32768),)
    assert all(R.small_plan(c, n, l).all_first for c in (8, 16) for n in (1, 16) for l in (20, 968)), "8-KB planes without the switch: <= 78 tiles"
    assert max(R.small_plan(c, n, l).tiles * n for c in (8, 16) for n in range(1, 17) for l in range(20, 20000, 44)
               if R.small_plan(c, n, l).PL == 8192) <= 80


def test_mid_plan_restates_filter_mid_hip():
    s = _src("filter_mid.hip")
    assert int(_one(r"constexpr int HALO = (\d+);", s)) == R.HALO
    assert int(_one(r"constexpr int NFP = (\d+);", s)) == R.MID_NFP
    assert int(_one(r"constexpr int BL = (\d+);", s)) == R.MID_BL
    assert _one(r"constexpr int NT = NTT, BL = ([^,]+),", s) == "64 * NT"
    assert int(_one(r"if \(nt_env \? nt_env == 2 : \(int64_t\)tiles \* N <= (\d+)\)", s)) == R.MID_SHORT_TILES
    assert int(_one(r"const bool small = \(int64_t\)tiles \* N <= (\d+);", s)) == R.FIRST_ONLY_TILES
    assert _one(r"ALIVE_CHECK_ARG\(\(double\)([^,]+) <= NFP,", s) == "BL * film_ld / L + 3.0"
    assert _one(r"constexpr int TT2 = ([^,]+),", s) == "128 - HALO"
    assert _one(r"for \(int sg = 1; sg <= \(([^)]+)\); \+\+sg\)", s) == "t256 < 64 ? t256 : 64"
    p = R.mid_plan(1, 800)                                             # the streaming step: four batch tiles -> twelve of 72 columns
    assert (p.NTT, p.TT, p.tiles, p.forms) == (2, 72, 12, ((True, 2, False, False),))
    p = R.mid_plan(128, 36000)
    assert (p.NTT, p.tiles, p.forms) == (4, 180, ((True, 4, False, False), (False, 4, False, False)))
    p = R.mid_plan(128, 36000, h16=True)                               # 140 batch tiles behind the first: two chip rounds of 4 segments
    assert p.sweep and p.forms[1] == (False, 4, True, True) and p.seg_cols % 256 == 0 and p.segments * p.seg_cols >= 36000 - 200
    p = R.mid_plan(17, 3204, h16=True)
    assert (p.tiles, p.sweep, p.segments, p.seg_cols) == (17, True, 12, 256)
    assert not R.mid_plan(1, 3204, h16=True).sweep and R.mid_plan(1, 3204, h16=True).forms == ((True, 4, True, False),)
    assert R.mid_plan(2, 1600).NTT == 2 and R.mid_plan(2, 1604).NTT == 4 and R.mid_plan(1, 1604, nt_env=4).NTT == 4


def test_the_cases_take_the_forms_they_name():
    """every accuracy and range case through the plans; the densest admitted tables are exactly at the launcher's bound, one frame more
    is refused; between them the cases reach every <C, FIRST, PL> that runs without a switch and the split <FIRST, NTT> forms"""
    small, mid = set(), set()
    for case in R.ACCURACY:
        p = case.plan()
        (mid if case.C == 64 else small).update(p.forms)
    assert small == {(c, first, pl) for c in (8, 16) for pl in (8192, 16384) for first in (True, False)} - {(8, False, 8192), (16, False, 8192)}
    assert mid == {(True, 2, False, False), (True, 4, False, False), (False, 4, False, False)}
    for c, n, l, lf in R.DENSEST:
        p = R.plan_for(c, n, l)
        assert p.frames_admitted(l, lf) and not p.frames_admitted(l, lf + 1)
        assert (256 if c == 64 else p.BL) * lf / l + 3.0 == (R.MID_NFP if c == 64 else R.SMALL_NFP)
        assert any(k.C == c and k.l == l and k.lf == lf and k.per_call == n for k in R.ACCURACY)
    for c, n, l, lf in R.SHORTEST:
        p = R.plan_for(c, n, l)
        assert p.frames_admitted(l, lf) and not R.plan_for(c, n, l - 4).frames_admitted(l - 4, lf) and p.tiles == 1
        assert any(k.C == c and k.l == l and k.lf == lf and k.per_call == n for k in R.ACCURACY)
    assert any(k.lf == 1 for k in R.ACCURACY) and any(k.l % k.lf for k in R.ACCURACY)
    for rc in R.RANGES:
        assert all((rc.up * rc.f0) % tt for tt in (72, 200, 456, 968)) or rc.f0 == 40
        p = R.plan_for(rc.C, rc.n, rc.up * rc.nf)
        assert p.frames_admitted(rc.up * rc.nf, rc.nf) and p.all_first == rc.range_all_first and rc.n * rc.C >= 256
        assert len(R.plan_for(rc.C, rc.n, rc.up * rc.frames).forms) == 2


# ---- sensitivity: every planted defect leaves the bars ---------------------------------------------------------------------------
def _keep(stage, v):
    return v["y"] if stage == "conv" else (v["sc"], v["sh"]) if stage == "film" else v


@lru_cache(maxsize=None)
def _sens_case(name, rng=None):
    case = next(k for k in R.ACCURACY if k.name == name)
    c = case.C
    sd, fw = R.block_weights(c)
    if rng is None:
        x, cnd, skip = R.inputs(c, case.l, case.lf, case.n)
        film, kw = R.film_table(cnd, fw), {}
    else:                                                              # frames f0 .. of a longer signal
        up = rng.up
        x, cnd, skip = R.inputs(c, up * rng.frames, rng.frames, rng.n)
        cut = slice(up * rng.f0, up * (rng.f0 + rng.nf))
        x, skip = x[:, :, cut], skip[:, :, cut]
        film, kw = R.film_table(cnd, fw)[:, :, rng.f0:rng.f0 + rng.nf], dict(t0=up * rng.f0, f0=rng.f0, frames=rng.frames)
    run = lambda **k: R.filter_block_split(x, film, R.PAD_ROWS, sd, "n", skip=skip, **kw, **k)
    return dict(key=case.key, plan=case.plan(), run=run, ex=run(rounding=False), a=run(flavour="f32"), b=run(flavour="f64"))


def _judge(s, hook):
    """the clean "f64" flavour passes every bar against the "f32" one; the same flavour with the defect does not -> its ratios"""
    assert not R.check_bars(R.profile_ratios(s["b"], s["a"], s["ex"]), s["key"])
    bad = s["run"](flavour="f64", hook=hook)
    r = R.profile_ratios(bad, s["a"], s["ex"])
    print(f"global {relerr(s['b'], s['ex']):.3e} -> {relerr(bad, s['ex']):.3e}; " + R.describe(r))
    assert R.check_bars(r, s["key"]), "the bars pass the defect"
    return r


@pytest.mark.parametrize("name", ["16-8k-l600", "8-8k-l460", "64-nt4-first"])
def test_one_tap_read_one_row_off_in_one_column_breaks_the_column_bar(name):
    """conv 5's third tap of channels 0 .. 7 reads the row before the right one, in the first output column of the second tile only: that
    one column leaves the bar, no other does"""
    s = _sens_case(name)
    col, j, d = s["plan"].TT, 2, 4

    def hook(stage, q, v):
        if stage == "conv" and q == 5:
            z, y = v["hi"] + v["lo"], v["y"].clone()
            src = col + (j - 4) * d
            y[:, :, col] += torch.einsum("oc,nc->no", v["w"][:, :8, j], z[:, :8, src - 1] - z[:, :8, src])
            return y
        return _keep(stage, v)
    r = _judge(s, hook)
    bar = R.BARS[s["key"]]["column"]
    assert r["column"][col] > 10 * bar[1]
    assert R.inside(torch.cat([r["column"][:col], r["column"][col + 1:]]), bar)


@pytest.mark.parametrize("name", ["16-8k-l204", "8-8k-l76", "64-nt2-l76"])
def test_a_reflection_off_by_one_breaks_the_column_bar(name):
    """conv 4 (dilation 4, the pad of 16) reflects column -k to k - 1 instead of k: the first columns leave the bar"""
    s = _sens_case(name)

    def hook(stage, q, v):
        return v["conv"](v["hi"], v["lo"], reflect_shift=-1) if stage == "conv" and q == 4 else _keep(stage, v)
    r = _judge(s, hook)
    bar = R.BARS[s["key"]]["column"]
    assert r["column"][:16].max() > 10 * bar[1] and R.inside(r["column"][R.HALO:], bar)


@pytest.mark.parametrize("name", ["16-8k-dense", "16-16k-dense", "8-8k-dense", "64-nt4-dense"])
def test_a_frame_clamped_one_early_at_a_tiles_end_breaks_the_column_bar(name):
    """at the largest frame density the launcher admits, the last 32 columns of the first tile take their lower frame no higher than the
    frame before the tile's last one (a staged table one frame short, i1 = i0 + 1 with it): the columns under the last frame leave the bar"""
    s = _sens_case(name)
    tt = s["plan"].TT
    cols = torch.arange(tt - 32, tt)

    def hook(stage, q, v):
        if stage != "film":
            return _keep(stage, v)
        i0 = v["i0"][cols]
        c0 = i0.clamp_max(int(i0.max()) - 1)
        w1 = v["w1"][cols]
        sc, sh = v["sc"].clone(), v["sh"].clone()
        sc[:, :, cols] = ((1.0 - w1) * v["S"][:, :, c0] + w1 * v["S"][:, :, c0 + 1]).to(sc.dtype)
        sh[:, :, cols] = ((1.0 - w1) * v["H"][:, :, c0] + w1 * v["H"][:, :, c0 + 1]).to(sh.dtype)
        return sc, sh
    r = _judge(s, hook)
    bar = R.BARS[s["key"]]["column"]
    assert r["column"][tt - 1] > 10 * bar[1] and R.inside(r["column"][:tt - 32], bar)


@pytest.mark.parametrize("name,group", [("16-16k-first", 1), ("8-8k-l460", 0), ("64-nt4-first", 5)])
def test_a_dropped_lo_plane_of_one_channel_group_breaks_the_bars(name, group):
    """conv 3 reads zeros for the lo plane of channels 8 g .. 8 g + 7 of its input: 2^-9 instead of 2^-17 on an eighth to all of one
    conv's operand -- every statistic leaves its bar"""
    s = _sens_case(name)

    def hook(stage, q, v):
        if stage == "conv_in" and q == 3:
            lo = v[1].clone()
            lo[:, 8 * group:8 * group + 8] = 0.0
            return v[0], lo
        return _keep(stage, v)
    r = _judge(s, hook)
    bars = R.BARS[s["key"]]
    assert r["total"] > 2 * bars["total"][1] and r["channel"].min() > bars["channel"][1] and r["peak"] > bars["peak"][1]


@pytest.mark.parametrize("name", ["16-16k-first", "8-8k-l460", "64-nt4-first"])
def test_w1_of_the_neighbouring_column_breaks_the_bars(name):
    """conv 2 interpolates its FiLM rows with the weight of the column before"""
    s = _sens_case(name)

    def hook(stage, q, v):
        if stage == "film" and q == 2:
            w1 = torch.roll(v["w1"], 1)
            return (1.0 - w1) * v["s0"] + w1 * v["s1"], (1.0 - w1) * v["h0"] + w1 * v["h1"]
        return _keep(stage, v)
    r = _judge(s, hook)
    assert r["total"] > 2 * R.BARS[s["key"]]["total"][1] and r["column"].median() > R.BARS[s["key"]]["column"][1]


@pytest.mark.parametrize("c", [8, 16, 64])
def test_a_table_column_computed_without_f0_breaks_the_bars(c):
    """range mode: conv 1 takes the table column of frame i as min(i, film_ld - 1) instead of i - f0 -- every column reads the table's
    last frame"""
    rng = next(r for r in R.RANGES if r.C == c and r.f0 == 37)
    s = _sens_case({8: "8-16k-rest", 16: "16-16k-rest", 64: "64-nt4-rest"}[c], rng)

    def hook(stage, q, v):
        if stage == "film" and q == 1:
            ld = v["S"].shape[2]
            c0, c1, w1 = v["i0"].clamp(0, ld - 1), v["i1"].clamp(0, ld - 1), v["w1"]
            return (1.0 - w1) * v["S"][:, :, c0] + w1 * v["S"][:, :, c1], (1.0 - w1) * v["H"][:, :, c0] + w1 * v["H"][:, :, c1]
        return _keep(stage, v)
    r = _judge(s, hook)
    assert r["total"] > 2 * R.BARS[s["key"]]["total"][1]


def test_a_result_more_accurate_than_the_split_product_breaks_the_lower_bars():
    """the fp32 oracle itself is not this kernel: it falls out of every bar at its lower end"""
    s = _sens_case("16-8k-l600")
    case = next(k for k in R.ACCURACY if k.name == "16-8k-l600")
    sd, _ = R.block_weights(16)
    x, cnd, skip = R.inputs(16, case.l, case.lf, case.n)
    oracle = O.filter_block(sd, "n", x, cnd) + skip
    r = R.profile_ratios(oracle, s["a"], s["ex"])
    bars = R.BARS["16"]
    assert r["column"].max() < bars["column"][0] and r["channel"].max() < bars["channel"][0] and r["total"] < bars["total"][0]
