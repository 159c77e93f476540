"""Host restatement of the fused split-bf16 FilterBlocks: csrc/filter_small.hip (C = 8, 16: alive_filter_block_small[_range]) and
csrc/filter_mid.hip (C = 64: alive_filter_block64[_range]), and the cases their tests share (tests/test_host_filter_split.py on the CPU,
tests/test_gpu_filter_split.py on the device).  The fp16 sweep kernel's twin is tools/filter_big_ref.py; what the two share (coordinates,
the reflected causal conv, the Abramowitz-Stegun GELU, the profile statistic, the weight constructors) is imported from there.

`small_plan` / `mid_plan` restate the launch rules: which plane size or how many column tiles per wave a call takes, its tile grid,
whether every tile runs the reflecting FIRST form, and for the fp16 form of the 64-channel block the sweep's segment split.
`filter_block_split` evaluates the whole block, input conv included, the way the kernels round it: every MFMA operand v is hi + lo with
hi = bf16(v), lo = bf16(v - hi), and a product is a_hi b_hi + a_hi b_lo + a_lo b_hi -- in one of two epilogue flavours, or exactly.

Why float64 IS a tight reference here, and what the two flavours are for.  A split operand carries 16 mantissa bits and the dropped
a_lo b_lo term is 2^-18 of the product: the chain has no coarse intermediate rounding whose flips would decorrelate two evaluations.
The error against the exact block is about 2^-17 per product and is a deterministic function of the operand values, which the
emulation reproduces; the flavours differ only in what comes on top (fp32 sums and adds, the erf polynomial's 1.5e-7, fused
multiply-adds).  The ratio of their error profiles against the exact block -- per column, per channel, in total, and of their largest
single errors -- over every accuracy case and seeds 0 .. 4 is the null band (NULL_BAND, measured by tests/test_host_filter_split.py); the
device -- hardware reciprocal and exp2, the MFMA's own summation order: one more realisation of the last bits -- has to lie inside that
band widened by 1.25 at each end (BARS).

Everything here is CPU torch; nothing touches the device.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from filter_big_ref import (COND, DILATIONS, NCONV, PAD_ROWS, WIDEN, _f32, _fma32, _gelu2_as, block_weights as _big_block_weights,  # noqa: F401
                            cdiv, film_table, gauss, lerp_coords)

HALO = 56                                      # causal reach of the six k5 convs: 4 (1 + 1 + 2 + 2 + 4 + 4), both files
SMALL_NFP = 10                                 # filter_small.hip::NFP: FiLM frames a tile may span
SMALL_PLANES = (8192, 16384, 32768)            # bytes per LDS plane: short signals, the batch default, PLANE_BATCH
SMALL_TINY_TILES = 16                          # at most so many PLANE_BATCH tiles: the 8-KB planes
MID_NFP = 8                                    # filter_mid.hip::NFP
MID_BL = 256                                   # filter_mid.hip::BL, the batch tile (NTT = 4); NTT = 2: 128
MID_SHORT_TILES = 16                           # at most so many batch tiles: NTT = 2
FIRST_ONLY_TILES = 256                         # at most so many tiles: every tile through the FIRST form, one launch (both files)
SAMPLES_PER_FRAME = {64: 80, 16: 160, 8: 320}  # at the decoder's scales


# ---- the launch rules ----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SmallPlan:
    """alive_filter_block_small_range + launch_small<C, PL>: filter_block_small_kernel<C, FIRST, PL> over `tiles` x N blocks"""
    C: int
    N: int
    L: int
    PL: int                                    # bytes per plane
    BL: int                                    # columns per tile, halo included
    TT: int                                    # output columns per tile
    tiles: int                                 # per window
    all_first: bool                            # one launch of <C, true, PL> over every tile; else tile 0 by it, the others by <C, false, PL>

    def frames_admitted(self, L, film_ld):
        """the launcher's bound on the frames under a tile (in double, as it computes it; a window shorter than a tile counts as a tile)"""
        return float(self.BL) * film_ld / L + 3.0 <= SMALL_NFP

    @property
    def forms(self):
        return ((self.C, True, self.PL),) if self.all_first or self.tiles == 1 else ((self.C, True, self.PL), (self.C, False, self.PL))


def small_tile(C, PL):
    """Cfg<C, PL>: (BL, TT)"""
    bl = PL // (2 * C)
    return bl, bl - HALO


def small_plan(C, N, L, plane_env=0):
    """plane_env: ALIVE_FBS_PLANE (0 = unset)"""
    assert C in (8, 16) and N > 0 and L > 16 and L % 4 == 0
    big_tiles = cdiv(L, small_tile(C, 32768)[1]) * N
    tiny = plane_env < 16384 if plane_env else big_tiles <= SMALL_TINY_TILES
    if not tiny and plane_env in (16384, 0):
        PL = 16384
    else:
        PL = 8192 if tiny else 32768
    BL, TT = small_tile(C, PL)
    tiles = cdiv(L, TT)
    return SmallPlan(C, N, L, PL, BL, TT, tiles, tiles * N <= FIRST_ONLY_TILES)


@dataclass(frozen=True)
class MidPlan:
    """filter_block64_impl<H16>: filter_block64_kernel<FIRST, NTT, H16, SWEEP>"""
    N: int
    L: int
    h16: bool
    NTT: int                                   # column tiles of 32 per wave
    BL: int
    TT: int
    tiles: int
    all_first: bool
    sweep: bool                                # the columns behind the first tile by <false, 4, true, true>
    segments: int = 0                          # sweep: blocks per window
    seg_cols: int = 0                          # sweep: columns per segment, a multiple of 256

    def frames_admitted(self, L, film_ld):
        """(the bound is the batch tile's whatever NTT)"""
        return float(MID_BL) * film_ld / L + 3.0 <= MID_NFP

    @property
    def forms(self):
        first = (True, self.NTT, self.h16, False)
        if self.all_first or self.tiles == 1:
            return (first,)
        return (first, (False, 4, True, True) if self.sweep else (False, 4, False, False))


def mid_plan(N, L, h16=False, nt_env=0):
    """nt_env: ALIVE_FB64_NT (0 = unset)"""
    assert N > 0 and L > 16 and L % 4 == 0
    tiles = cdiv(L, MID_BL - HALO)
    if (nt_env == 2) if nt_env else tiles * N <= MID_SHORT_TILES:
        return MidPlan(N, L, h16, 2, 128, 128 - HALO, cdiv(L, 128 - HALO), True, False)
    small = tiles * N <= FIRST_ONLY_TILES
    if small or tiles == 1 or not h16:
        return MidPlan(N, L, h16, 4, MID_BL, MID_BL - HALO, tiles, small, False)
    rem = L - (MID_BL - HALO)
    t256 = cdiv(rem, MID_BL)
    best_s, best_cost = 1, -1
    for sg in range(1, min(t256, 64) + 1):     # the fewest chip rounds x (tiles per segment + the warm-up tile)
        cost = cdiv(N * sg, 256) * (cdiv(t256, sg) + 1)
        if best_cost < 0 or cost < best_cost:
            best_cost, best_s = cost, sg
    seg_cols = cdiv(t256, best_s) * MID_BL
    return MidPlan(N, L, h16, 4, MID_BL, MID_BL - HALO, tiles, False, True, cdiv(rem, seg_cols), seg_cols)


def plan_for(C, N, L, plain=False):
    return mid_plan(N, L, plain) if C == 64 else small_plan(C, N, L)


# ---- the block ---------------------------------------------------------------------------------------------------------------
def split2(v):
    """(hi, lo) of an MFMA operand as float64: hi = bf16(v), lo = bf16(v - hi), round to nearest even both times -- module/_pack.py's
    split of the weights (split_bf16, pack_filter_small), the kernels' pack2 / pack2s of a column"""
    hi = v.to(torch.bfloat16).double()
    lo = (v.double() - hi).to(torch.bfloat16).double()
    return hi, lo


def _unfold(z, d, taps, reflect_shift):
    """[N][C][L] -> [taps C][N L]: row (j, c) holds z[c][t + (j - 4) d] for the last `taps` of five taps, the signal reflected on its left
    (column -k reads column k + reflect_shift)"""
    n, c, l = z.shape
    t = torch.arange(-4 * d, l)
    zp = z[:, :, torch.where(t < 0, -t + reflect_shift, t)]
    return torch.stack([zp[:, :, j * d:j * d + l] for j in range(5 - taps, 5)], 0).permute(0, 2, 1, 3).reshape(taps * c, n * l)


def split_conv(zh, zl, wh, wl, b, d, reflect_shift=0):
    """reflect-left causal conv at dilation d (weights [Co][C][taps <= 5]: the last taps of a k5 conv; taps 1 = a 1x1 conv) of the split
    product: sum over taps of wh zh + wh zl + wl zh, + bias, in float64, as one GEMM (zl None: one exact operand zh, wh)"""
    n, _, l = zh.shape
    co, c, taps = wh.shape
    flat = lambda w: w.permute(0, 2, 1).reshape(co, taps * c)
    if zl is None:
        y = flat(wh) @ _unfold(zh, d, taps, reflect_shift)
    else:
        y = torch.cat([flat(wh + wl), flat(wh)], 1) @ torch.cat([_unfold(zh, d, taps, reflect_shift), _unfold(zl, d, taps, reflect_shift)], 0)
    return y.reshape(co, n, l).permute(1, 0, 2) + b.view(1, -1, 1)


def filter_block_split(x, film, film_off, sd, prefix, skip=None, t0=0, f0=0, frames=None, flavour="f32", rounding=True, hook=None):
    """The whole FilterBlock as ops.filter_block_small / ops.filter_block64 take it: x [N][C][L] the block's input, film [N][rows][film_ld]
    the fp32 FiLM table (rows film_off + q 2 C + (scale of C channels | shift of C channels) for conv q), reference-layout weights
    sd[prefix + ".input_conv.weight / bias"], sd[prefix + ".blocks.j.c1 / c2.conv.conv.weight / bias"], skip added behind the block.
    t0 / f0 / frames: the window is columns t0 .. of a signal with `frames` frames, and the table holds frames f0 .. f0 + film_ld - 1 of it
    (frames outside are clamped to the table's edge, as the kernels clamp them); the start is reflected at the window's own column 0.
    -> float64 [N][C][L].

    rounding=True: the weights, the raw input columns and every modulated conv input gelu(v) * interp(scale) + interp(shift) are split
    into hi + lo bf16 planes, a product is a_hi b_hi + a_hi b_lo + a_lo b_hi, interpolation coordinates in fp32.  flavour "f64":
    everything else in float64 with the exact erf GELU.  flavour "f32": conv sums rounded to fp32, residual adds and the epilogue in
    fp32 in the kernels' operation order (scale rows halved, Abramowitz-Stegun erf, fused multiply-adds).  rounding=False: the exact
    float64 block (float64 coordinates).

    hook(stage, q, value) -> value lets a test plant a defect (q = -1: the input conv):
      ("film", q, dict(sc, sh, s0, s1, h0, h1, w1, i0, i1, col0, col1, S, H)) -> (sc, sh) the interpolated rows of conv q [N][C][L]; S / H
          its scale / shift rows of the table [N][C][film_ld], i0 / i1 the signal's frames, col0 / col1 the table's columns;
      ("conv_in", q, (hi, lo)) -> (hi, lo) the operand planes of conv q (lo None without rounding);
      ("conv", q, dict(hi, lo, y, w, conv)) -> y its output; w = the weights hi + lo, conv(hi, lo, reflect_shift=0) recomputes it."""
    assert flavour in ("f64", "f32")
    single = rounding and flavour == "f32"
    n, c, l = x.shape
    film_ld = film.shape[2]
    Lf = film_ld if frames is None else frames
    i0, i1, w1 = lerp_coords(l, film_ld, l, t0, Lf, rounding)
    col0 = (i0 - f0).clamp(0, film_ld - 1)
    col1 = (i1 - f0).clamp(0, film_ld - 1)
    w0 = (1.0 - w1.to(torch.float32)).double() if rounding else 1.0 - w1

    def conv_of(q, z):
        if q < 0:
            w, b, d = sd[prefix + ".input_conv.weight"].double(), sd[prefix + ".input_conv.bias"].double(), 0
        else:
            j, cc = q // 2, ("c1", "c2")[q & 1]
            w, b, d = sd[f"{prefix}.blocks.{j}.{cc}.conv.conv.weight"].double(), sd[f"{prefix}.blocks.{j}.{cc}.conv.conv.bias"].double(), DILATIONS[q]
        if rounding:
            wh, wl = split2(w.float())
            zh, zl = split2(z.float() if single else z)
        else:
            wh, wl, zh, zl = w, None, z, None
        if hook is not None:
            zh, zl = hook("conv_in", q, (zh, zl))
        conv = lambda a, b_, reflect_shift=0: split_conv(a, b_, wh, wl, b, d, reflect_shift)
        y = conv(zh, zl)
        if hook is not None:
            y = hook("conv", q, dict(hi=zh, lo=zl, y=y, w=wh if wl is None else wh + wl, conv=conv))
        return _f32(y) if single else y

    h = conv_of(-1, _f32(x) if rounding else x.double())
    v = h
    for q in range(NCONV):
        rows = film[:, film_off + q * 2 * c:film_off + (q + 1) * 2 * c].double()
        S, H = rows[:, :c], rows[:, c:]
        s0, s1, h0, h1 = S[:, :, col0], S[:, :, col1], H[:, :, col0], H[:, :, col1]
        if single:
            W0, W1 = _f32(w0), _f32(w1)
            sc = _fma32(W0, _f32(0.5 * s0), W1 * _f32(0.5 * s1))              # the staged table holds scale / 2
            sh = _fma32(W0, _f32(h0), W1 * _f32(h1))
        else:
            sc = w0 * s0 + w1 * s1
            sh = w0 * h0 + w1 * h1
        if hook is not None:
            sc, sh = hook("film", q, dict(sc=sc, sh=sh, s0=s0, s1=s1, h0=h0, h1=h1, w1=w1, i0=i0, i1=i1, col0=col0, col1=col1, S=S, H=H))
        if single:
            z = _fma32(_gelu2_as(v), _f32(sc), _f32(sh))
        else:
            z = v * 0.5 * (1.0 + torch.special.erf(v * math.sqrt(0.5))) * sc + sh
        v = conv_of(q, z)
        if q & 1:
            h = v + h                                                         # (an fp32 add in the "f32" flavour)
            v = h
    out = h
    if skip is not None:
        out = out + (_f32(skip) if single else skip.double())
    return out.double()


# ---- the statistic ---------------------------------------------------------------------------------------------------------
def error_profile(out, exact):
    """dict(column, channel, total, peak) of out - exact: rms per column pooled over windows and channels, rms per channel pooled over
    windows and columns, the total rms, and the largest single error in units of its channel's rms in the exact block"""
    exact = exact.double()
    e2 = (out.double() - exact).pow_(2)
    rms2 = exact.pow(2).mean(dim=(0, 2), keepdim=True)
    return dict(column=e2.mean(dim=(0, 1)).sqrt(), channel=e2.mean(dim=(0, 2)).sqrt(), total=e2.mean().sqrt().item(),
                peak=(e2 / rms2).max().sqrt().item())


def profile_ratios(a, b, exact):
    """error_profile(a) / error_profile(b), statistic by statistic"""
    pa, pb = error_profile(a, exact), error_profile(b, exact)
    return {k: pa[k] / pb[k] for k in pa}


def inside(r, bar):
    r = torch.as_tensor(r, dtype=torch.float64)
    return bool((r >= bar[0]).all() and (r <= bar[1]).all())


def check_bars(r, key):
    """every ratio of profile_ratios inside BARS[key]; -> the failures as text"""
    bad = []
    for stat, bar in BARS[key].items():
        v = torch.as_tensor(r[stat], dtype=torch.float64).reshape(-1)
        if not inside(v, bar):
            bad.append(f"{stat}: {v.min().item():.4f} (at {int(v.argmin())}) .. {v.max().item():.4f} (at {int(v.argmax())}) outside "
                       f"{bar[0]:.4f} .. {bar[1]:.4f}")
    return bad


def describe(r):
    return (f"column {r['column'].min():.4f} .. {r['column'].max():.4f}, channel {r['channel'].min():.4f} .. {r['channel'].max():.4f}, "
            f"total {r['total']:.4f}, peak {r['peak']:.4f}")


# ---- the cases -----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """n windows of l columns with lf frames, run in calls of `group` windows (0: one call): the launch rules pick the form by the
    call's tile count, so the forms for short signals take a handful of windows per call, while a column's rms wants n C >= 256 values"""
    name: str
    C: int
    n: int
    l: int
    lf: int
    form: tuple                                # what the plan of a call has to say: (PL or NTT, all_first)
    group: int = 0

    @property
    def per_call(self):
        return self.group or self.n

    @property
    def key(self):
        return str(self.C)

    def plan(self):
        p = plan_for(self.C, self.per_call, self.l)
        assert ((p.NTT if self.C == 64 else p.PL), p.all_first) == self.form, (self.name, p)
        assert self.n % self.per_call == 0 and self.n * self.C >= 256
        assert p.frames_admitted(self.l, self.lf), (self.name, "refused by the launcher")
        return p


# The launchers take L > 16, but bound BL lf / L + 3 by NFP even where the window has fewer than BL columns (tests/test_gpu_fine_scale_fusion.py
# pins that refusal for the fused stores): with one frame the shortest lengths taken are L = 40 (C = 16, 256-column tiles), 76 (C = 8, 512)
# and 52 (C = 64, 256).
ACCURACY = [
    # C = 16 on 8-KB planes (TT 200): the shortest length taken (one frame), one vector past a tile, exactly three tiles
    Case("16-8k-l40", 16, 16, 40, 1, (8192, True)),
    Case("16-8k-l204", 16, 16, 204, 2, (8192, True)),
    Case("16-8k-l600", 16, 16, 600, 5, (8192, True)),
    # 16-KB planes (TT 456), every tile FIRST, 130.86 samples per frame; then 6 x 52 > 256 tiles: FIRST + <16, false, 16384>
    Case("16-16k-first", 16, 17, 916, 7, (16384, True)),
    Case("16-16k-rest", 16, 52, 2284, 14, (16384, False)),
    # the largest frame density admitted, exactly at the bound (BL lf / L + 3 = 10)
    Case("16-8k-dense", 16, 16, 1024, 28, (8192, True), group=8),
    Case("16-16k-dense", 16, 18, 1024, 14, (16384, True), group=9),
    # C = 8 on 8-KB planes (TT 456): at most 16 windows per call
    Case("8-8k-l76", 8, 32, 76, 1, (8192, True), group=16),
    Case("8-8k-l460", 8, 32, 460, 3, (8192, True), group=16),
    Case("8-16k-rest", 8, 32, 8716, 27, (16384, False)),                   # TT 968: 10 x 32 tiles, 322.8 samples per frame
    Case("8-8k-dense", 8, 32, 2048, 28, (8192, True), group=8),
    # C = 64, split form: NTT 2 (TT 72), NTT 4 all FIRST (80.8 samples per frame), 9 x 33 tiles: FIRST + <false, 4, false>, the density bound
    Case("64-nt2-l52", 64, 4, 52, 1, (2, True)),
    Case("64-nt2-l76", 64, 4, 76, 1, (2, True)),
    Case("64-nt2-l220", 64, 4, 220, 3, (2, True)),
    Case("64-nt4-first", 64, 17, 404, 5, (4, True)),
    Case("64-nt4-rest", 64, 33, 1604, 20, (4, False)),
    Case("64-nt4-dense", 64, 4, 1024, 20, (4, True)),
]
# one frame more than the densest admitted: (C, windows per call, L, lf)
DENSEST = [(16, 8, 1024, 28), (16, 9, 1024, 14), (8, 8, 2048, 28), (64, 4, 1024, 20)]
# the shortest windows taken with one frame: one vector of four columns less is refused
SHORTEST = [(16, 16, 40, 1), (8, 16, 76, 1), (64, 4, 52, 1)]


@dataclass(frozen=True)
class RangeCase:
    """frames f0 .. f0 + nf - 1 of a signal of `frames` frames at the scale's samples per frame, given only those FiLM columns"""
    C: int
    n: int
    frames: int
    f0: int
    nf: int
    range_all_first: bool                      # the range run's tiles all take the FIRST form (the whole signal's never do)

    @property
    def up(self):
        return SAMPLES_PER_FRAME[self.C]

    @property
    def margins(self):
        """inside them a range run is the whole run's samples: the first columns interpolate towards frame f0 - 1 and the reflected
        start reaches 56 columns further; the last frame's partner lies outside the table"""
        up = self.up
        return up // 2 + 1 + HALO, up * self.nf - up - up // 2 - 1


# frames 40 .. 89 of 128, and a range that starts inside a tile of every form (37 x 80, 160, 320 is no multiple of 72, 200, 456 or 968)
RANGES = [RangeCase(8, 32, 128, 40, 50, False), RangeCase(16, 16, 128, 40, 50, False), RangeCase(64, 8, 128, 40, 50, True),
          RangeCase(8, 32, 128, 37, 27, False), RangeCase(16, 16, 128, 37, 27, True), RangeCase(64, 8, 128, 37, 27, True)]


# The null band: the smallest and the largest ratio of the two rounding flavours' statistics (either over the other) over every
# ACCURACY case of the key and seeds 0 .. 4, as tests/test_host_filter_split.py measures them on the host; BARS = the band widened by
# 1.25 at each end: what the device has to meet.
NULL_BAND = {
    # measured: column 0.8053 .. 1.2417, channel 0.9761 .. 1.0245, total 0.9919 .. 1.0081, peak 0.8176 .. 1.2230
    "8": dict(column=(0.80, 1.25), channel=(0.97, 1.03), total=(0.99, 1.01), peak=(0.81, 1.23)),
    # measured: column 0.8390 .. 1.1919, channel 0.9019 .. 1.1088, total 0.9603 .. 1.0414, peak 0.7349 .. 1.3608
    "16": dict(column=(0.83, 1.20), channel=(0.90, 1.11), total=(0.96, 1.05), peak=(0.73, 1.37)),
    # measured: column 0.8400 .. 1.1905, channel 0.8997 .. 1.1115, total 0.9885 .. 1.0116, peak 0.7822 .. 1.2785
    "64": dict(column=(0.83, 1.20), channel=(0.89, 1.12), total=(0.98, 1.02), peak=(0.78, 1.28)),
}
BARS = {k: {s: (lo / WIDEN, hi * WIDEN) for s, (lo, hi) in v.items()} for k, v in NULL_BAND.items()}


def block_weights(c, seed=7):
    """filter_big_ref.block_weights with a real input conv"""
    sd, fw = _big_block_weights(c, seed)
    sd["n.input_conv.weight"] = gauss(f"fsr.iw{c}", (c, c, 1), seed, 1.0 / np.sqrt(c))
    sd["n.input_conv.bias"] = gauss(f"fsr.ib{c}", (c,), seed, 0.1)
    return sd, fw


def inputs(c, l, lf, n, seed=7):
    """x, conditioning, skip (torch's seeded CPU generator: these tensors are the large ones)"""
    g = torch.Generator().manual_seed(((seed * 131 + c) * 1000003 + l) * 131 + lf)
    return torch.randn(n, c, l, generator=g), torch.randn(n, COND, lf, generator=g), torch.randn(n, c, l, generator=g)
