"""Host restatement of the fused fp16 FilterBlock of csrc/filter_big.hip (filter_block256_kernel behind alive_filter_block256_fp16,
alive_filter_block64s_fp16 and alive_filter_block64s_fp16_up), and the cases its tests share (tests/test_host_filter_big.py on the
CPU, tests/test_gpu_filter_big.py on the device).

`sweep_plan` restates fb_launch: the batch is one sequence of tiles, window after window, and block b takes the run
b * per_block .. of them; a run that starts inside a window begins with an unstored warm-up tile, a window's first tile reflects its
own columns.  `filter_block_fp16` evaluates the block without its input conv the way the kernel rounds it -- fp16 weights, every
modulated conv input saturated and rounded to fp16 -- in one of two epilogue flavours, or exactly (rounding=False).

Why two flavours.  A float64 evaluation on the same fp16 operands is NO tight pointwise reference for the chain: the intermediate fp16
roundings flip between any two evaluations whose epilogues differ in the last fp32 bits, and two such evaluations differ from each
other by as much as either differs from the exact block.  What an emulation does predict is the kernel's noise PROFILE: the rms error
against the exact block per column (pooled over windows and channels) and per channel (pooled over windows and columns).  The two
flavours are two independent realisations of the flips; the ratio of their profiles, over every accuracy case and several seeds, is
the null band (NULL_BAND, measured by tests/test_host_filter_big.py), and the device's result -- fp32 MFMA sums, hardware
reciprocal and exp2: one more realisation -- has to lie inside that band widened by 1.25 at each end (BARS).  Extra error confined to
a few columns or to a wave's channel group, which the global rms figure hides, stands out of it.

Everything here is CPU torch; nothing touches the device.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

NCONV = 6
CTX = 16
DILATIONS = (1, 1, 2, 2, 4, 4)
F16_MAX = 65504.0


def cdiv(a, b):
    return (a + b - 1) // b


def tile_columns(C):
    """Geo<C>::BL"""
    return {256: 128, 64: 512}[C]


def table_frames(C):
    """Geo<C>::NFS: the frames a wave's FiLM table holds"""
    return {256: 16, 64: 8}[C]


def ratio_admitted(C, L, frames):
    """fb_launch's bound on the frames under a wave's 128 columns"""
    return min(L, 128) * frames / L + 3.0 <= table_frames(C)


# ---- the sweep -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Run:
    block: int
    g0: int                                    # the block's stored tiles g0 .. g1 - 1 of the batch's tile sequence
    g1: int
    warm: bool                                 # begins with the unstored tile g0 - 1 (g0 lies inside a window)
    firsts: tuple                              # its tiles that are a window's first (reflected context)

    @property
    def crossings(self):
        """window starts inside the run: a `first` tile behind another tile of the same block"""
        return sum(1 for g in self.firsts if g > self.g0)


@dataclass(frozen=True)
class Plan:
    N: int
    L: int
    C: int
    cus: int
    BL: int
    tiles: int
    total: int
    per_block: int
    blocks: int
    runs: tuple

    @property
    def warm_runs(self):
        return sum(1 for r in self.runs if r.warm)

    @property
    def crossing_runs(self):
        return sum(1 for r in self.runs if r.crossings)

    @property
    def most_window_starts(self):
        return max(len(r.firsts) for r in self.runs)

    @property
    def last_is_short(self):
        return self.runs[-1].g1 - self.runs[-1].g0 < self.per_block

    def workspace_bytes(self):
        """what the launch needs (the _workspace_bytes queries answer for one block per tile: never less)"""
        return self.blocks * NCONV * CTX * 2 * self.C


def sweep_plan(N, L, C, cus):
    BL = tile_columns(C)
    tiles = cdiv(L, BL)
    total = N * tiles
    per_block = cdiv(total, cus)
    blocks = cdiv(total, per_block)
    runs = []
    for b in range(blocks):
        g0 = b * per_block
        g1 = min(g0 + per_block, total)
        runs.append(Run(b, g0, g1, g0 % tiles != 0, tuple(g for g in range(g0, g1) if g % tiles == 0)))
    return Plan(N, L, C, cus, BL, tiles, total, per_block, blocks, tuple(runs))


@dataclass(frozen=True)
class SweepCase:
    name: str
    C: int
    L: int
    lf: int                                    # frames of the window (film_ld)
    per_block: int
    up: bool = False
    skip: bool = True
    short_last: bool = False                   # the last block holds fewer tiles than the others
    window_starts: int = 1                     # some run holds at least so many window starts
    rng: tuple = None                          # (t0, f0, frames of the whole signal)

    @property
    def warm_possible(self):
        """a run can start inside a window unless per_block is a multiple of the tiles per window: then every run starts at a window's
        first tile whatever N is (L = 200: runs of 6 tiles over windows of 2)"""
        return self.per_block % cdiv(self.L, tile_columns(self.C)) != 0


# the sweep regimes of the GPU file: tens of columns short of a tile, runs over several windows, the long window of the product
SWEEPS = [
    SweepCase("256-l520", 256, 520, 52, 3, short_last=True),                 # 5 tiles, the last 8 columns wide
    SweepCase("256-l200", 256, 200, 5, 6, skip=False, short_last=True, window_starts=3),
    SweepCase("256-l4500", 256, 4500, 45, 5, skip=False),
    SweepCase("64-l1300", 64, 1300, 16, 2),
    SweepCase("64-l600", 64, 600, 8, 5, short_last=True),
    SweepCase("64-l1300-up", 64, 1300, 16, 2, up=True),
    SweepCase("64-l600-up", 64, 600, 8, 5, up=True, skip=False, short_last=True),
    SweepCase("256-range", 256, 520, 52, 3, rng=(1300, 130, 450)),           # columns 1300 .. 1819 of a 4500-column signal
    SweepCase("64-range", 64, 1280, 16, 2, rng=(3200, 40, 450)),             # columns 3200 .. 4479 of a 36000-column signal
]


def windows_for(case, cus):
    """the smallest batch that puts `case` into its regime on `cus` compute units: per_block as named, a run that starts inside a
    window (where one can), a run that crosses a window boundary, the short last block and the window starts per run the case names"""
    tiles = cdiv(case.L, tile_columns(case.C))
    for N in range(1, cdiv(case.per_block * cus, tiles) + 1):
        p = sweep_plan(N, case.L, case.C, cus)
        if p.per_block != case.per_block:
            continue
        if plan_fits(case, p):
            return N
    raise AssertionError(f"{case.name}: no batch reaches per_block {case.per_block} with the case's properties on {cus} CUs")


def plan_fits(case, p):
    return (p.per_block == case.per_block and (p.warm_runs > 0) == case.warm_possible and p.crossing_runs > 0
            and (not case.short_last or p.last_is_short) and p.most_window_starts >= case.window_starts)


def check_plan(case, p):
    """the properties every sweep case asserts before it launches"""
    covered = [g for r in p.runs for g in range(r.g0, r.g1)]
    assert covered == list(range(p.total)), "the runs partition the tile sequence"
    assert p.per_block == case.per_block, (p.per_block, case.per_block)
    assert p.per_block > 1 and p.blocks <= p.cus
    if case.warm_possible:
        assert p.warm_runs > 0, "no run starts inside a window"
    else:
        assert p.warm_runs == 0
    assert p.crossing_runs > 0, "no run crosses a window boundary"
    assert p.most_window_starts >= case.window_starts
    if case.short_last:
        assert p.last_is_short
    assert ratio_admitted(case.C, case.L, case.lf)
    return p


# ---- the block ---------------------------------------------------------------------------------------------------------------
def _f32(x):
    return x.to(torch.float32)


def _fma32(a, b, c):
    """fmaf on fp32 tensors: the product is exact in float64, the sum is rounded there once and once more to fp32 (the double
    rounding differs from one rounding in about 2^-29 of the cases: these flavours only need to be plausible last-bit realisations)"""
    return (a.double() * b.double() + c.double()).to(torch.float32)


def lerp_coords(L, ratio_num, ratio_den, t0, Lf, single):
    """F.interpolate(mode="linear") coordinates of columns t0 .. t0 + L - 1 (csrc/common.h::lerp_coord; ATen's
    area_pixel_compute_source_index): (i0, i1, w1).  single: in fp32 with ratio = float(num) / float(den), as the kernel and ATen on
    fp32 tensors compute them; else in float64, as ATen on float64 tensors."""
    t = torch.arange(L, dtype=torch.float64) + t0
    if single:
        ratio = (torch.tensor(float(ratio_num), dtype=torch.float32) / torch.tensor(float(ratio_den), dtype=torch.float32)).double()
        src = (ratio * (t + 0.5) - 0.5).to(torch.float32).double()
    else:
        src = (float(ratio_num) / float(ratio_den)) * (t + 0.5) - 0.5
    src = src.clamp_min(0.0)
    i0 = src.floor().long().clamp_max(Lf - 1)
    i1 = (i0 + 1).clamp_max(Lf - 1)
    return i0, i1, src - i0.double()                     # (exact in either precision)


def _gelu2_as(x):
    """2 gelu(x) = x + |x| erf(|x| / sqrt 2) on fp32, Abramowitz-Stegun 7.1.26 in the kernel's operation order (emit_tile), the
    hardware reciprocal replaced by IEEE division"""
    one = torch.ones((), dtype=torch.float32)
    c = lambda v: torch.tensor(v, dtype=torch.float32)
    ax = x.abs()
    tq = _fma32(ax, c(0.3275911) * c(0.70710678118654752440), one)
    t = one / tq
    xs = x * c(0.84932180028801904272)
    ex = torch.exp2(-(xs * xs))
    p = _fma32(c(1.061405429), t, c(-1.453152027))
    p = _fma32(p, t, c(1.421413741))
    p = _fma32(p, t, c(-0.284496736))
    p = _fma32(p, t, c(0.254829592))
    erf_abs = _fma32(-(p * t), ex, one)
    return _fma32(ax, erf_abs, x)


def causal_conv(z, w, b, d):
    """reflect-left causal k5 conv at dilation d in float64: z [N][C][L], w [Co][C][5], b [Co]"""
    n, _, l = z.shape
    zp = F.pad(z, (4 * d, 0), mode="reflect")
    y = b.view(1, -1, 1).expand(n, w.shape[0], l).clone()
    for j in range(5):
        y += torch.matmul(w[:, :, j], zp[:, :, j * d:j * d + l])
    return y


def filter_block_fp16(x, film, film_off, sd, prefix, skip=None, up=None, t0=0, f0=0, frames=None, flavour="f32", rounding=True,
                      hook=None):
    """The FilterBlock WITHOUT its input conv, as ops.filter_block256 takes it: x [N][C][L] the residual stream, film [N][rows][film_ld]
    the fp32 FiLM table (rows film_off + q 2 C + (scale of C channels | shift of C channels) for conv q), reference-layout weights
    sd[prefix + ".blocks.j.c1 / c2.conv.conv.weight / bias"], skip added behind the block, up = (weight [64][16][2], bias [16]) the
    ConvTranspose1d(64, 16, 2, 2) behind that.  t0 / f0 / frames: the window is columns t0 .. of a signal with `frames` frames, and
    the table holds frames f0 .. f0 + film_ld - 1 of it (frames outside are clamped to the table's edge, as the kernel clamps them).
    -> float64 [N][C][L] or [N][16][2 L].

    rounding=True: weights rounded to fp16, every modulated conv input gelu(v) * interp(scale) + interp(shift) saturated at +-65504
    and rounded to fp16, interpolation coordinates in fp32.  flavour "f64": everything else in float64 with the exact erf GELU.
    flavour "f32": conv sums rounded to fp32, residual adds and the epilogue in fp32 in the kernel's operation order (scale rows
    halved, Abramowitz-Stegun erf, fused multiply-adds).  rounding=False: the exact float64 block (float64 coordinates).

    hook(stage, q, value) -> value lets a test plant a defect: ("film", q, dict(sc, sh, s0, s1, h0, h1, w1)) -> (sc, sh) the
    interpolated rows of conv q [N][C][L]; ("conv_in", q, z) the rounded input of conv q; ("conv", q, dict(z, y, conv)) -> y its output,
    conv(z) recomputes it."""
    assert flavour in ("f64", "f32")
    single = rounding and flavour == "f32"
    n, c, l = x.shape
    film_ld = film.shape[2]
    Lf = film_ld if frames is None else frames
    i0, i1, w1 = lerp_coords(l, film_ld, l, t0, Lf, rounding)
    col0 = (i0 - f0).clamp(0, film_ld - 1)
    col1 = (i1 - f0).clamp(0, film_ld - 1)
    w0 = (1.0 - w1.to(torch.float32)).double() if rounding else 1.0 - w1
    h = _f32(x) if single else x.double()
    v = h
    for q in range(NCONV):
        j, cc = q // 2, ("c1", "c2")[q & 1]
        rows = film[:, film_off + q * 2 * c:film_off + (q + 1) * 2 * c].double()
        s0, s1, h0, h1 = rows[:, :c, col0], rows[:, :c, col1], rows[:, c:, col0], rows[:, c:, col1]
        if single:
            W0, W1 = _f32(w0), _f32(w1)
            sc = _fma32(W0, _f32(0.5 * s0), W1 * _f32(0.5 * s1))            # the table holds scale / 2
            sh = _fma32(W0, _f32(h0), W1 * _f32(h1))
        else:
            sc = w0 * s0 + w1 * s1
            sh = w0 * h0 + w1 * h1
        if hook is not None:
            sc, sh = hook("film", q, dict(sc=sc, sh=sh, s0=s0, s1=s1, h0=h0, h1=h1, w1=w1))
        if single:
            z = _fma32(_gelu2_as(v), sc, sh).double()
        else:
            z = v * 0.5 * (1.0 + torch.special.erf(v * math.sqrt(0.5))) * sc + sh
        if rounding:
            z = z.clamp(-F16_MAX, F16_MAX).to(torch.float16).double()
        if hook is not None:
            z = hook("conv_in", q, z)
        w = sd[f"{prefix}.blocks.{j}.{cc}.conv.conv.weight"].double()
        b = sd[f"{prefix}.blocks.{j}.{cc}.conv.conv.bias"].double()
        if rounding:
            w = w.clamp(-F16_MAX, F16_MAX).to(torch.float16).double()
        conv = lambda zz, w=w, b=b, d=DILATIONS[q]: causal_conv(zz, w, b, d)
        y = conv(z)
        if hook is not None:
            y = hook("conv", q, dict(z=z, y=y, conv=conv))
        v = _f32(y) if single else y
        if q & 1:
            h = v + h                                                     # (fp32 add in the "f32" flavour)
            v = h
    out = h
    if skip is not None:
        out = out + (_f32(skip) if single else skip.double())
    out = out.double()
    if up is not None:
        out = F.conv_transpose1d(out, up[0].double(), up[1].double(), stride=2)
        if single:
            out = _f32(out).double()
    return out


# ---- the statistic ---------------------------------------------------------------------------------------------------------
def column_profile(out, exact):
    """rms error per column, pooled over windows and channels"""
    return (out.double() - exact.double()).pow(2).mean(dim=(0, 1)).sqrt()


def channel_profile(out, exact):
    """rms error per channel, pooled over windows and columns"""
    return (out.double() - exact.double()).pow(2).mean(dim=(0, 2)).sqrt()


def total_error(out, exact):
    return (out.double() - exact.double()).pow(2).mean().sqrt().item()


def profile_ratios(a, b, exact):
    """(per column, per channel, total) of error(a) / error(b)"""
    return (column_profile(a, exact) / column_profile(b, exact), channel_profile(a, exact) / channel_profile(b, exact),
            total_error(a, exact) / total_error(b, exact))


# ---- the accuracy cases ------------------------------------------------------------------------------------------------------
# (C, l, lf, n, up): lengths that are no multiple of the tile, one column past a tile, one tile exactly, the shortest windows; then
# the ratio edges fb_launch admits: the most frames per 128 columns, a non-integer samples-per-frame ratio
ACCURACY = [
    (256, 370, 37, 2, False), (256, 130, 13, 2, False), (256, 1280, 128, 1, False), (256, 33, 4, 3, False), (256, 128, 13, 2, False),
    (256, 129, 13, 2, False), (256, 1280, 130, 1, False), (256, 1000, 97, 1, False),
    (64, 1200, 15, 3, False), (64, 520, 6, 1, False), (64, 512, 6, 2, False), (64, 513, 6, 2, False), (64, 40, 2, 3, False),
    (64, 1200, 15, 2, True), (64, 1280, 50, 1, False),
]
COND = 24
PAD_ROWS = 5                                   # the block's FiLM rows start inside a larger table, as in the decoder


def bars_key(C, up):
    return "64up" if up else str(C)


# The null band: the smallest and the largest ratio of the two rounding flavours' profiles (either over the other) over every
# ACCURACY case of the key and seeds 0 .. 4, as tests/test_host_filter_big.py measures them; a column pools N C values (N 16 with `up`),
# which is why the 64-channel bands are the wider ones.  BARS = the band widened by 1.25 at each end: what the device has to meet.
NULL_BAND = {
    # measured: column 0.8533 .. 1.1719, channel 0.8304 .. 1.2042, total 0.9908 .. 1.0093
    "256": dict(column=(0.85, 1.18), channel=(0.82, 1.21), total=(0.99, 1.01)),
    # measured: column 0.7400 .. 1.3513, channel 0.9093 .. 1.0998, total 0.9914 .. 1.0087
    "64": dict(column=(0.73, 1.36), channel=(0.90, 1.11), total=(0.99, 1.01)),
    # measured: column 0.7202 .. 1.3885, channel 0.9883 .. 1.0119, total 0.9978 .. 1.0022
    "64up": dict(column=(0.71, 1.40), channel=(0.98, 1.02), total=(0.99, 1.01)),
}
WIDEN = 1.25
BARS = {k: {s: (lo / WIDEN, hi * WIDEN) for s, (lo, hi) in v.items()} for k, v in NULL_BAND.items()}


def gauss(name, shape, seed=7, scale=1.0):
    from module import synthetic
    return synthetic.gaussian(name, seed, shape, scale)


def block_weights(c, seed=7):
    """reference-layout weights of a FilterBlock (identity input conv, for the oracle) and the (weight, bias, post_add) of the 1x1 conv
    that makes its FiLM table from the conditioning"""
    sd = {"n.input_conv.weight": torch.eye(c).unsqueeze(-1).contiguous(), "n.input_conv.bias": torch.zeros(c)}
    ws, bs, post = [torch.zeros(PAD_ROWS, COND, 1)], [torch.zeros(PAD_ROWS)], [torch.zeros(PAD_ROWS)]
    for j in range(3):
        for cc in ("c1", "c2"):
            p = f"n.blocks.{j}.{cc}"
            sd[p + ".conv.conv.weight"] = gauss(p + f"w{c}", (c, c, 5), seed, 0.5 / np.sqrt(c))
            sd[p + ".conv.conv.bias"] = gauss(p + f"b{c}", (c,), seed, 0.1)
            sd[p + ".to_scale.weight"] = gauss(p + f"sw{c}", (c, COND, 1), seed, 0.1)
            sd[p + ".to_scale.bias"] = gauss(p + f"sb{c}", (c,), seed, 0.1)
            sd[p + ".to_shift.weight"] = gauss(p + f"hw{c}", (c, COND, 1), seed, 0.1)
            sd[p + ".to_shift.bias"] = gauss(p + f"hb{c}", (c,), seed, 0.1)
            ws += [sd[p + ".to_scale.weight"], sd[p + ".to_shift.weight"]]
            bs += [sd[p + ".to_scale.bias"], sd[p + ".to_shift.bias"]]
            post += [torch.ones(c), torch.zeros(c)]
    return sd, (torch.cat(ws, 0), torch.cat(bs, 0), torch.cat(post))


def up_weights(seed=7):
    """ConvTranspose1d(64, 16, 2, 2): weight [Ci][Co][r], bias"""
    return gauss("fbr.upw", (64, 16, 2), seed, 0.12), gauss("fbr.upb", (16,), seed, 0.1)


def accuracy_inputs(c, l, lf, n, seed=7):
    """x, conditioning, skip of an accuracy case: the construction of test_fused_filter_block_256"""
    return (gauss(f"fbr.x{c}.{l}", (n, c, l), seed), gauss(f"fbr.c{c}.{l}", (n, COND, lf), seed), gauss(f"fbr.s{c}.{l}", (n, c, l), seed))


def film_table(cnd, fw):
    """the FiLM table on the host in fp32 (the device tests take alive_conv1d's: the block reads whichever it is given)"""
    return F.conv1d(cnd.float(), fw[0], fw[1]) + fw[2].view(1, -1, 1)
