"""Host twin of tests/test_gpu_filter_big.py: the restatement of the fused fp16 FilterBlock (tools/filter_big_ref.py; the kernel is
csrc/filter_big.hip) is pinned to the oracle, the sweep regimes the GPU file asks for are proved reachable on several CU counts, the null
band behind the GPU file's profile bars is measured, and the bars are shown to catch defects that the global rms check lets pass.

The statistic: the rms error against the exact float64 block per column (pooled over windows and channels) and per channel (pooled
over windows and columns).  Two emulations of the kernel's roundings with different last-bit behaviour in their epilogues give the same
profile within the null band; a defect confined to a few columns or to a 32-channel group does not.
"""
import os
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
import filter_big_ref as R                                           # noqa: E402

SEEDS = (0, 1, 2, 3, 4)
GLOBAL_BOUND = 6e-4                            # test_fused_filter_block_256's check, which every planted defect has to pass


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)).item()


# ---- the exact flavour is the oracle's block -----------------------------------------------------------------------------
def _double_case(c, l, lf, n):
    sd, fw = R.block_weights(c)
    x, cnd, skip = R.accuracy_inputs(c, l, lf, n)
    sd64 = {k: v.double() for k, v in sd.items()}
    film = F.conv1d(cnd.double(), fw[0].double(), fw[1].double()) + fw[2].double().view(1, -1, 1)
    return sd64, x.double(), cnd.double(), skip.double(), film


@pytest.mark.parametrize("c,l,lf,n", [(256, 130, 13, 2), (256, 33, 4, 2), (256, 1000, 97, 1), (64, 600, 8, 2), (64, 40, 2, 1)])
def test_the_exact_flavour_is_the_oracles_filter_block(c, l, lf, n):
    """rounding=False with an identity input conv against O.filter_block on float64 tensors: the FiLM rows at their offset in a larger
    table, ATen's float64 interpolation, the reflected causal convs at dilations 1, 1, 2, 2, 4, 4, the residual behind every second one"""
    sd64, x, cnd, skip, film = _double_case(c, l, lf, n)
    ref = O.filter_block(sd64, "n", x, cnd) + skip
    out = R.filter_block_fp16(x, film, R.PAD_ROWS, sd64, "n", skip=skip, rounding=False)
    assert out.dtype == torch.float64 and out.shape == ref.shape
    assert (out - ref).abs().max().item() <= 1e-12 * ref.pow(2).mean().sqrt().item()
    if c == 64 and l >= 512:
        w, b = (t.double() for t in R.up_weights())
        up = R.filter_block_fp16(x, film, R.PAD_ROWS, sd64, "n", skip=skip, up=(w, b), rounding=False)
        want = F.conv_transpose1d(ref, w, b, stride=2)
        assert up.shape == (n, 16, 2 * l) and (up - want).abs().max().item() <= 1e-12 * want.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("c", [256, 64])
def test_the_exact_flavour_in_a_frame_range_is_the_whole_signals_columns(c):
    """frames 40 .. 89 of a 128-frame signal from a table that holds those frames only (t0 / f0 / frames): past the reach of the window's
    reflected start (56 columns, + the columns that interpolate towards frame 39) and short of its last frame the samples are the
    oracle's on the whole signal"""
    lf, f0, nf = 128, 40, 50
    up = 10 if c == 256 else 80
    sd64, x, cnd, skip, film = _double_case(c, up * lf, lf, 1)
    whole = O.filter_block(sd64, "n", x, cnd) + skip
    cut = slice(up * f0, up * (f0 + nf))
    part = R.filter_block_fp16(x[:, :, cut], film[:, :, f0:f0 + nf], R.PAD_ROWS, sd64, "n", skip=skip[:, :, cut], t0=up * f0, f0=f0,
                               frames=lf, rounding=False)
    lo, hi = up // 2 + 1 + 56, up * nf - up - up // 2 - 1
    scale = whole.pow(2).mean().sqrt().item()
    assert (part[:, :, lo:hi] - whole[:, :, up * f0 + lo:up * f0 + hi]).abs().max().item() <= 1e-12 * scale
    assert (part[:, :, :16] - whole[:, :, up * f0:up * f0 + 16]).abs().max().item() > 1e-3 * scale      # (the reflected start is the window's own)
    again = R.filter_block_fp16(x, film, R.PAD_ROWS, sd64, "n", skip=skip, rounding=False)                 # (and without the range arguments)
    assert (again - whole).abs().max().item() <= 1e-12 * scale


def test_the_rounding_flavours_round_what_the_kernel_rounds():
    """both flavours sit at one fp16 plane's distance from the exact block (2^-12 per operand: 3.6 .. 4.4e-4 of the output at these
    depths), closer to each other than to it, and are not the same numbers; a planted 1e6 saturates instead of overflowing"""
    c, l, lf, n = 64, 600, 8, 2
    sd, fw = R.block_weights(c)
    x, cnd, skip = R.accuracy_inputs(c, l, lf, n)
    film = R.film_table(cnd, fw)
    ex = R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", skip=skip, rounding=False)
    a = R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", skip=skip, flavour="f32")
    b = R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", skip=skip, flavour="f64")
    assert 2e-4 < relerr(a, ex) < GLOBAL_BOUND and 2e-4 < relerr(b, ex) < GLOBAL_BOUND
    assert 0 < relerr(a, b) < relerr(a, ex)
    x[1, 3, 77] = 1e6
    assert torch.isfinite(R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", flavour="f32")).all()


# ---- the sweep plan ------------------------------------------------------------------------------------------------------
def test_sweep_plan_restates_the_launcher():
    """the bench's shape on 256 CUs (192 windows x 36 tiles = 27 per CU) and the hand-worked small ones"""
    p = R.sweep_plan(192, 4500, 256, 256)
    assert (p.BL, p.tiles, p.total, p.per_block, p.blocks) == (128, 36, 6912, 27, 256)
    p = R.sweep_plan(9, 4490, 256, 256)                                # the one shape of test_fused_filter_block_256 beyond per_block 1
    assert (p.tiles, p.per_block, p.blocks) == (36, 2, 162)
    p = R.sweep_plan(3, 1300, 64, 4)
    assert (p.BL, p.tiles, p.total, p.per_block, p.blocks) == (512, 3, 9, 3, 3) and p.warm_runs == 0 and p.crossing_runs == 0
    p = R.sweep_plan(3, 1300, 64, 2)                                   # runs 0 .. 4 and 5 .. 8: the second starts at window 1's last tile
    assert [(r.g0, r.g1, r.warm, r.firsts) for r in p.runs] == [(0, 5, False, (0, 3)), (5, 9, True, (6,))]
    assert p.crossing_runs == 2 and p.last_is_short and p.most_window_starts == 2


@pytest.mark.parametrize("cus", [256, 64, 128, 304])
@pytest.mark.parametrize("case", R.SWEEPS, ids=lambda s: s.name)
def test_every_sweep_case_reaches_its_regime(case, cus):
    """the batch tests/test_gpu_filter_big.py derives from the device's CU count puts the case into the regime it names: the runs
    partition the tile sequence, per_block is the named one, a run starts inside a window (behind a warm-up tile), a run crosses a window
    boundary (a reflected `first` tile in its middle), the last block is short where the case says so.  The kernel's own loop -- from
    g0 - 1 where g0 lies inside a window -- stores every tile exactly once."""
    n = R.windows_for(case, cus)
    p = R.check_plan(case, R.sweep_plan(n, case.L, case.C, cus))
    stored = []
    for b in range(p.blocks):                                          # filter_block256_kernel's tile loop
        g0 = b * p.per_block
        g1 = min(g0 + p.per_block, p.total)
        for g in range(g0 - 1 if g0 % p.tiles else g0, g1):
            if g >= g0:
                stored.append(g)
            else:
                assert g // p.tiles == g0 // p.tiles                   # the warm-up tile is the same window's
    assert stored == list(range(p.total))
    assert n <= cus // p.tiles * p.per_block + p.per_block             # (the small-group calls: a handful)
    if cus == 256:                                                     # the inputs stay small: x, skip and the FiLM table
        assert n * case.C * case.L * 4 < 150e6
        assert n * case.C * case.L * 4 * (2 if case.skip else 1) + n * (12 * case.C + R.PAD_ROWS) * case.lf * 4 < 200e6
    assert p.workspace_bytes() <= n * p.tiles * R.NCONV * R.CTX * 2 * case.C


def test_the_l200_case_cannot_start_a_run_inside_a_window():
    """runs of 6 tiles over windows of 2: every run starts at a window's first tile for any batch -- the case is there for its three
    window starts per run, and says so"""
    case = next(s for s in R.SWEEPS if s.name == "256-l200")
    assert not case.warm_possible
    assert all(R.sweep_plan(n, 200, 256, 256).warm_runs == 0 for n in range(641, 769))
    assert all(s.warm_possible for s in R.SWEEPS if s is not case)


# ---- the null band and the bars ----------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _flavours(c, l, lf, n, up, seed):
    sd, fw = R.block_weights(c, seed)
    x, cnd, skip = R.accuracy_inputs(c, l, lf, n, seed)
    film = R.film_table(cnd, fw)
    upw = R.up_weights(seed) if up else None
    kw = dict(skip=skip, up=upw)
    return (R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", rounding=False, **kw),
            R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", flavour="f32", **kw),
            R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", flavour="f64", **kw))


def _both_ways(r):
    r = torch.as_tensor(r, dtype=torch.float64).reshape(-1)
    return min(r.min().item(), (1.0 / r).min().item()), max(r.max().item(), (1.0 / r).max().item())


def test_the_null_band_of_two_emulations_lies_inside_the_recorded_one():
    """every accuracy case of the GPU file x five seeds: the ratio of the two rounding flavours' column profiles, channel profiles and
    total errors against the exact block, either flavour over the other.  The extremes are the null band; the recorded constants
    (tools/filter_big_ref.py::NULL_BAND, rounded outwards to two decimals) still contain them, and BARS is that band widened by 1.25."""
    band = {}
    for (c, l, lf, n, up) in R.ACCURACY:
        assert R.ratio_admitted(c, l, lf)
        for seed in SEEDS:
            ex, a, b = _flavours(c, l, lf, n, up, seed)
            assert relerr(a, ex) < GLOBAL_BOUND and relerr(b, ex) < GLOBAL_BOUND
            d = band.setdefault(R.bars_key(c, up), dict(column=[9.0, 0.0], channel=[9.0, 0.0], total=[9.0, 0.0]))
            for stat, r in zip(("column", "channel", "total"), R.profile_ratios(a, b, ex)):
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


# ---- sensitivity: defects the global check passes, the bars do not ---------------------------------------------------------
def _keep(stage, v):
    return v["y"] if stage == "conv" else (v["sc"], v["sh"]) if stage == "film" else v


@lru_cache(maxsize=None)
def _sens_case(l, lf, n, smooth):
    c = 256
    sd, fw = R.block_weights(c)
    x, cnd, skip = R.accuracy_inputs(c, l, lf, n)
    if smooth:                                                         # a conditioning that drifts by 0.005 per frame
        cnd = R.gauss("fbr.smooth0", (n, R.COND, 1)) + 0.005 * R.gauss("fbr.smooth1", (n, R.COND, 1)) * torch.arange(lf, dtype=torch.float32)
    film = R.film_table(cnd, fw)
    oracle = O.filter_block(sd, "n", x, cnd) + skip                    # the fp32 oracle of test_fused_filter_block_256
    ex = R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", skip=skip, rounding=False)
    a = R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", skip=skip, flavour="f32")
    b = R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", skip=skip, flavour="f64")
    return dict(sd=sd, x=x, skip=skip, film=film, oracle=oracle, ex=ex, a=a, b=b)


def _inside(r, bar):
    return bool((r >= bar[0]).all() and (r <= bar[1]).all())


def _judge(case, bad):
    """(global figure of the defective result, column ratios, channel ratios against the clean "f32" flavour); the clean "f64" flavour
    passes every bar on the same inputs"""
    col, ch, tot = R.profile_ratios(case["b"], case["a"], case["ex"])
    bars = R.BARS["256"]
    assert _inside(col, bars["column"]) and _inside(ch, bars["channel"]) and bars["total"][0] <= tot <= bars["total"][1]
    e = relerr(bad, case["oracle"])
    col, ch, _ = R.profile_ratios(bad, case["a"], case["ex"])
    print(f"global {relerr(case['b'], case['oracle']):.3e} -> {e:.3e}; column ratio {col.min():.2f} .. {col.max():.2f}, "
          f"channel ratio {ch.min():.2f} .. {ch.max():.2f}")
    assert e < GLOBAL_BOUND, e                                         # the present check passes it
    return col, ch


def test_a_stale_chunk_in_a_context_row_breaks_the_column_bar():
    """the tile that starts at column 384 of window 0 finds, in the context row 16 columns back of the last conv's input, one 16-byte
    chunk (channels 40 .. 47) left over from the tile before (the row 128 columns earlier): every output channel of ONE column is off by
    ~0.09, the global figure moves from 3.7e-4 to 5.6e-4 of 6e-4"""
    case = _sens_case(4500, 450, 2, False)
    s, back, ch0 = 384, 16, 40

    def hook(stage, q, v):
        if stage == "conv" and q == 5:
            z = v["z"].clone()
            z[0, ch0:ch0 + 8, s - back] = z[0, ch0:ch0 + 8, s - back - 128]
            y = v["y"].clone()
            y[:, :, s:] = v["conv"](z)[:, :, s:]                       # (the tile before read the row while it was right)
            return y
        return _keep(stage, v)
    bad = R.filter_block_fp16(case["x"], case["film"], R.PAD_ROWS, case["sd"], "n", skip=case["skip"], flavour="f64", hook=hook)
    col, _ = _judge(case, bad)
    assert col[s] > 10 * R.BARS["256"]["column"][1]
    assert _inside(torch.cat([col[:s], col[s + 1:]]), R.BARS["256"]["column"])


def test_film_rows_left_uninterpolated_at_a_tiles_end_break_the_column_bar():
    """conv 3 takes the FiLM rows of the last two frames' columns of the tile 128 .. 255 from the lower frame alone (a table one frame
    short), under a conditioning that drifts by 0.005 per frame: the global figure moves from 4.1e-4 to 4.7e-4"""
    case = _sens_case(370, 37, 3, True)
    cols = slice(236, 256)

    def hook(stage, q, v):
        if stage == "film" and q == 3:
            sc, sh = v["sc"].clone(), v["sh"].clone()
            sc[:, :, cols], sh[:, :, cols] = v["s0"][:, :, cols].to(sc.dtype), v["h0"][:, :, cols].to(sh.dtype)
            return sc, sh
        return _keep(stage, v)
    bad = R.filter_block_fp16(case["x"], case["film"], R.PAD_ROWS, case["sd"], "n", skip=case["skip"], flavour="f64", hook=hook)
    col, _ = _judge(case, bad)
    assert col[cols].max() > R.BARS["256"]["column"][1]
    assert not _inside(col, R.BARS["256"]["column"])


def test_added_error_on_eight_columns_breaks_the_column_bar():
    """2e-3 rms (8.7e-4 of the output's rms: the size of the fp16 noise itself is 8.7e-4 x 0.43) on columns 120 .. 127 of every window"""
    case = _sens_case(370, 37, 3, False)
    bad = case["b"].clone()
    bad[:, :, 120:128] += R.gauss("fbr.noise8", tuple(bad[:, :, 120:128].shape)).double() * 2e-3
    col, ch = _judge(case, bad)
    assert col[120:128].min() > R.BARS["256"]["column"][1]
    assert _inside(torch.cat([col[:120], col[128:]]), R.BARS["256"]["column"])
    assert _inside(ch, R.BARS["256"]["channel"])                       # (spread over all channels it is no channel defect)


def test_a_defect_confined_to_one_waves_channels_breaks_the_channel_bar():
    """2e-3 rms on channels 96 .. 127 -- wave 3's of the eight -- at every column: the global figure stays below 6e-4, the column profile
    moves by a factor the column bar allows, every one of the 32 channels leaves the channel bar"""
    case = _sens_case(370, 37, 3, False)
    bad = case["b"].clone()
    bad[:, 96:128] += R.gauss("fbr.noise32", tuple(bad[:, 96:128].shape)).double() * 2e-3
    col, ch = _judge(case, bad)
    assert ch[96:128].min() > R.BARS["256"]["channel"][1]
    assert _inside(torch.cat([ch[:96], ch[128:]]), R.BARS["256"]["channel"])


def test_a_result_without_the_fp16_rounding_breaks_the_lower_bars():
    """more accurate than one fp16 plane is not this kernel: the fp32 oracle itself falls out of every bar at its lower end"""
    case = _sens_case(370, 37, 3, False)
    col, ch, tot = R.profile_ratios(case["oracle"], case["a"], case["ex"])
    bars = R.BARS["256"]
    assert col.max() < bars["column"][0] and ch.max() < bars["channel"][0] and tot < bars["total"][0]
