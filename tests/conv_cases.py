"""Operands, references and the case matrix of the exact-operand tests of alive_conv1d (csrc/conv.hip, conv_split.hip,
conv_skinny.hip).  NumPy and torch on the CPU only; the library is not imported here.  tests/test_host_conv_operands.py proves on
the CPU what the generators promise, tests/test_gpu_conv_exact.py runs the matrix on the device.

The idea: operands for which every product and every partial sum is an fp32 number.  Then the sum does not depend on its order, so
the tiled, the split and the few-column kernel must all return the BITS of an integer computation; the tolerance is zero and any
error of indexing, halo, padding, tail, tile edge or linear epilogue is a mismatch at a named element.

  regime "I"    x, w, bias, post_add, residual, skip: small integers times a power of two, ch_scale a signed power of two.  Exact in
                bf16, fp16 and fp32; every lo plane is zero.  Every precision.
  regime "IIw"  w = a + b 2^-10 (a in +-{1, 2}, b = sign(a) {0 .. 3}): hi = bf16(w) = a and lo = b 2^-10 exactly, the third plane is zero;
                x integer.  "IIx": the same with the roles exchanged.  bf16x3 and bf16x6 (and fp32).
  regime "IIwx" both operands split.  bf16x3 on the split kernel only: the expected value is the THREE-product sum
                sum(a1 a2 + (a1 b2 + a2 b1) 2^-10), in units of 2^-10 -- the kernel drops lo x lo, and exactly that.
In every regime |bias| + sum |w| |x| and what the epilogue adds stay below 2^24 of the smallest unit in use (checked on the CPU).

With an activation v itself is still exact and the only error left is the function's own; the bounds below are derived from the
functions' definitions, not measured:
  erff-GELU, expf, sinf (exact kernel, few-column kernel; expf on the split kernel too)   |y - f(v)| <= 2^-21 max(|v|, |f(v)|)
  gelu_fast / gelu_fast2 (split kernel; the second output Z everywhere)   |y - gelu(v)| <= 4e-7 |v| + 2^-22 |gelu(v)|
      (Abramowitz-Stegun 7.1.26's 1.5e-7, the 1-ulp v_rcp_f32 / v_exp_f32, three fp32 roundings)
  every add of the linear epilogue behind an activation rounds once: 2^-24 of its result; ch_scale is a power of two and exact
  Z = gelu(v) sc + sh    |z - .| <= |sc| (tol_gelu(v) + 1.13 err(v)) + 2^-22 (|gelu(v) sc| + |sh|), gelu' <= 1.13; err(v) = 0
      without an activation in front; sc, sh = F.interpolate(mode="linear") of the fp32 FiLM rows"""
import itertools
import math
import zlib
from dataclasses import dataclass, replace

import numpy as np
import torch
import torch.nn.functional as F

SKINNY_COLS = 96          # alive_conv1d: N * Tout <= 96 -> conv_skinny.hip (not for plain fp16, plane operands or a frame range)
EP = ("post_add", "ch_scale", "residual", "skip")
EP_SUBSETS = [tuple(e for e, on in zip(EP, bits) if on) for bits in itertools.product((0, 1), repeat=4)]
NPLANES = {"fp32": 0, "bf16x3": 2, "bf16x6": 3, "fp16": 1}


def pad16(v):
    return (v + 15) // 16 * 16


def pad32(v):
    return (v + 31) // 32 * 32


@dataclass(frozen=True)
class Case:
    kernel: str               # the kernel alive_conv1d's dispatch must choose: "exact" | "split" | "skinny"
    prec: str                 # "fp32" | "bf16x3" | "bf16x6" | "fp16"
    n: int
    ci: int
    co: int                   # output channels (transposed: the GEMM has co * r rows)
    tin: int
    kw: int = 1
    stride: int = 1
    dil: int = 1
    pad: int = 0
    mode: int = 0
    out_len: int = 0          # 0: the natural length
    r: int = 0                # ConvTranspose1d(k == stride == r); 0: a conv
    ep: tuple = ()
    act: str = None
    lf: int = 0               # FiLM frames; 0: no second output
    want_raw: bool = True
    regime: str = "I"
    xa: int = 3               # |x| <= xa (the integer part)
    wa: int = 3               # |w| <= wa (regime I: integers, times 2^wexp)
    wexp: int = 0
    hot: int = 0              # > 0: every weight of the channels from `hot` up is +-1 (the wrapped-index cases)
    xp: bool = False          # plane-packed input (AliveConv.Xp)
    zp: bool = False          # plane-packed second output (AliveConv.Zp)
    yp: int = 0               # AliveConv.Yp: 1 fp16 plane / 2 bf16 planes
    tag: str = ""

    @property
    def rows(self):
        return self.co * self.r if self.r else self.co

    @property
    def tout(self):
        if self.r:
            return self.tin
        return self.out_len or (self.tin + self.pad - self.dil * (self.kw - 1) - 1) // self.stride + 1

    @property
    def cols(self):
        return self.n * self.tout

    @property
    def K(self):
        return self.ci * (1 if self.r else self.kw)

    @property
    def id(self):
        s = f"{self.tag}-{self.prec}-{self.regime}-n{self.n}ci{self.ci}co{self.co}t{self.tin}"
        if self.r:
            s += f"r{self.r}"
        else:
            s += f"k{self.kw}s{self.stride}d{self.dil}p{self.pad}m{self.mode}o{self.tout}"
        if self.ep:
            s += "-" + "+".join(e[:2] for e in self.ep)
        if self.act:
            s += "-" + self.act
        if self.lf:
            s += f"-lf{self.lf}" + ("" if self.want_raw else "zonly")
        for f in ("xp", "zp", "yp"):
            if getattr(self, f):
                s += f"-{f}{int(getattr(self, f))}"
        return s

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())


def dispatch(c):
    """the kernel alive_conv1d chooses for the case, from its dispatch rules: at most 96 columns -> the few-column kernel (unless
    plain fp16 or plane operands), otherwise the split kernel by precision, otherwise the exact kernel by its rows"""
    rows = c.rows
    if c.cols <= SKINNY_COLS and c.prec != "fp16" and not c.xp and not c.zp:
        kw = 1 if c.r else c.kw
        kp = pad16(c.ci * kw) if c.prec == "fp32" else kw * pad32(c.ci)
        pw = kw == 1 and c.stride == 1 and c.pad == 0 and c.tout <= c.tin
        return f"skinny/np{NPLANES[c.prec]}/{'pw' if pw else 'gen'}/waves{16 if kp >= 512 else 8}"
    if c.prec != "fp32":
        return f"split/bm{128 if rows > 64 else 64}/np{NPLANES[c.prec]}" + ("/xp" if c.xp else "")
    if rows > 64:
        return "exact/bm128"
    if rows > 16:
        return "exact/bm64" + ("/ypl" if c.yp else "")
    upv = c.r in (2, 4) and c.act is None and "post_add" not in c.ep and "ch_scale" not in c.ep
    return "exact/bm16" + ("/upv" if upv else "")


# ---------------------------------------------------------------------------------------------------------------- operands ----
def _ints(rng, shape, a):
    return torch.from_numpy(rng.integers(-a, a + 1, size=shape)).double()


def _split_vals(rng, shape):
    """a + b 2^-10 with a in +-{1, 2} and b = sign(a) {0 .. 3}: bf16(a + b 2^-10) = a, since half an ulp of bf16 just above 1 is
    2^-8 = 4 x 2^-10 (b of the other sign would fall into the binade below a power of two, where half an ulp is 2 x 2^-10)"""
    a = torch.from_numpy(rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=shape))
    b = torch.from_numpy(rng.integers(0, 4, size=shape)).double() * a.sign()
    return a, b


def make(c):
    """the case's operands as float64 CPU tensors (each an fp32 number), in ops.conv1d's layouts: x [n][ci][tin], w [co][ci][kw] (or
    [ci][co][r] transposed), bias [co], post_add / ch_scale [rows], residual / skip [n][co][tout], film [n][2 rows + 3][lf] with the
    scale rows from 1 and the shift rows from rows + 2.  `unit`: every value up to the activation is a multiple of it."""
    rng = np.random.default_rng(c.seed)
    u = 2.0 ** c.wexp
    wshape = (c.ci, c.co, c.r) if c.r else (c.co, c.ci, c.kw)
    xshape = (c.n, c.ci, c.tin)
    o = {"unit": u}
    if c.regime in ("IIw", "IIwx"):
        a, b = _split_vals(rng, wshape)
        o["w"], o["w_hi"], o["w_lo"] = a + b / 1024.0, a, b / 1024.0
        o["unit"] = 2.0 ** -10
    else:
        o["w"] = _ints(rng, wshape, c.wa) * u
        o["w_hi"], o["w_lo"] = o["w"], torch.zeros(wshape, dtype=torch.float64)
    if c.regime in ("IIx", "IIwx"):
        a, b = _split_vals(rng, xshape)
        o["x"], o["x_hi"], o["x_lo"] = a + b / 1024.0, a, b / 1024.0
        o["unit"] = 2.0 ** -10
    else:
        o["x"] = _ints(rng, xshape, c.xa)
        o["x_hi"], o["x_lo"] = o["x"], torch.zeros(xshape, dtype=torch.float64)
    if c.hot:
        sl = (slice(c.hot, None),) if c.r else (slice(None), slice(c.hot, None))
        o["w"][sl] = torch.from_numpy(rng.choice(np.array([-1.0, 1.0]), size=tuple(o["w"][sl].shape)))
        o["w_hi"] = o["w"]
    bu = u if c.regime == "I" else 1.0
    o["bias"] = _ints(rng, (c.co,), 4) * bu
    if "post_add" in c.ep:
        o["post_add"] = _ints(rng, (c.rows,), 3) * bu
    if "ch_scale" in c.ep:
        e = rng.integers(-1 if c.regime == "I" else 0, 2, size=(c.rows,))
        o["ch_scale"] = torch.from_numpy(rng.choice(np.array([-1.0, 1.0]), size=(c.rows,)) * 2.0 ** e)
        if c.regime == "I":
            o["unit"] = o["unit"] / 2.0
    for k in ("residual", "skip"):
        if k in c.ep:
            o[k] = _ints(rng, (c.n, c.co, c.tout), 8) * bu
    if c.lf:
        o["film"] = torch.from_numpy(rng.standard_normal((c.n, 2 * c.rows + 3, c.lf))).float()
        o["film_scale_row"], o["film_shift_row"] = 1, c.rows + 2
    return o


# -------------------------------------------------------------------------------------------------------------- references ----
def source_index(c):
    """[tout][kw] input sample of (column, tap) after padding, and whether it exists: pad_mode 0 zero-fills both sides, 1 reflects
    on the left (-i) and zero-fills on the right, 2 reflects on both sides (2 (Tin - 1) - i on the right)"""
    t = torch.arange(c.tout).view(-1, 1)
    j = torch.arange(c.kw).view(1, -1)
    i = t * c.stride + j * c.dil - c.pad
    if c.mode != 0:
        i = torch.where(i < 0, -i, i)
    if c.mode == 2:
        i = torch.where(i >= c.tin, 2 * (c.tin - 1) - i, i)
    ok = (i >= 0) & (i < c.tin)
    return torch.where(ok, i, torch.zeros_like(i)), ok


def padded(c, x):
    """the signal the conv reads, written out: sample u of it is input sample u - pad under the case's pad_mode, long enough
    for every tap of the last column"""
    U = (c.tout - 1) * c.stride + (c.kw - 1) * c.dil + 1
    i = torch.arange(U) - c.pad
    if c.mode != 0:
        i = torch.where(i < 0, -i, i)
    if c.mode == 2:
        i = torch.where(i >= c.tin, 2 * (c.tin - 1) - i, i)
    ok = (i >= 0) & (i < c.tin)
    return x[:, :, torch.where(ok, i, torch.zeros_like(i))] * ok.to(x.dtype)


def lin(c, w, x):
    """the bias-free conv / transposed conv in float64 through torch"""
    w, x = w.double(), x.double()
    if c.r:
        return F.conv_transpose1d(x, w, None, stride=c.r)
    return F.conv1d(padded(c, x), w, None, stride=c.stride, dilation=c.dil)


def lin_int(c, w, x):
    """the same sum on int64 operands, index by index (source_index), without torch's conv"""
    assert w.dtype == torch.int64 and x.dtype == torch.int64
    if c.r:
        return torch.einsum("nit,ior->notr", x, w).reshape(c.n, c.co, c.tin * c.r)
    i, ok = source_index(c)
    xg = x[:, :, i] * ok.to(torch.int64)                       # [n][ci][tout][kw]
    return torch.einsum("nitj,oij->not", xg, w)


def per_row(c, vec):
    """a [rows] vector of the epilogue as it meets the output [co][tout * r]: row co * r + j is sample t * r + j of channel co"""
    if not c.r:
        return vec.view(1, -1, 1)
    return vec.view(c.co, 1, c.r).expand(c.co, c.tin, c.r).reshape(1, c.co, c.tin * c.r)


def conv_value(c, o):
    """v before the activation, exact in float64: the full product, or for bf16x3 on the split kernel the three plane products"""
    if c.kernel == "split" and c.prec == "bf16x3":
        v = lin(c, o["w_hi"], o["x_hi"]) + lin(c, o["w_hi"], o["x_lo"]) + lin(c, o["w_lo"], o["x_hi"])
    else:
        v = lin(c, o["w"], o["x"])
    return v + o["bias"].view(1, -1, 1)


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def tol_gelu_fast(v):
    return 4e-7 * v.abs() + 2.0 ** -22 * gelu64(v).abs()


def activation(c, v):
    """f(v) in float64 and the bound of the device function's own error"""
    if c.act is None:
        return v, torch.zeros_like(v)
    f = {"gelu": gelu64, "exp": torch.exp, "sin": torch.sin}[c.act](v)
    if c.act == "gelu" and c.kernel == "split":
        return f, tol_gelu_fast(v)
    return f, 2.0 ** -21 * torch.maximum(v.abs(), f.abs())


def film_rows(c, o):
    """interpolated FiLM scale and shift [n][rows][tout] (fp32 arithmetic of F.interpolate), as float64"""
    f = o["film"]
    sc = F.interpolate(f[:, o["film_scale_row"]:o["film_scale_row"] + c.rows], size=c.tout, mode="linear", align_corners=False)
    sh = F.interpolate(f[:, o["film_shift_row"]:o["film_shift_row"] + c.rows], size=c.tout, mode="linear", align_corners=False)
    return sc.double(), sh.double()


def reference(c, o):
    """{"v", "y", "yerr", ["z", "zerr"]}: float64.  yerr == 0 everywhere <=> the output is exact and compared bit for bit.
    Order of conv_epilogue.h: act, + post_add, * ch_scale, + residual, + skip."""
    v = conv_value(c, o)
    y, err = activation(c, v)
    for k in EP:
        if k not in c.ep:
            continue
        if k == "ch_scale":
            s = per_row(c, o[k])
            y, err = y * s, err * s.abs()
        else:
            y = y + (per_row(c, o[k]) if k == "post_add" else o[k])
            if c.act is not None:
                err = err + 2.0 ** -24 * y.abs()
    out = {"v": v, "y": y, "yerr": err}
    if c.lf:
        sc, sh = film_rows(c, o)
        g = gelu64(y)
        out["z"] = g * sc + sh
        out["zerr"] = sc.abs() * (tol_gelu_fast(y) + 1.13 * err) + 2.0 ** -22 * ((g * sc).abs() + sh.abs())
    return out


def unit_sum_bound(c, o):
    """the largest magnitude any partial sum (and, without an activation, any stage of the epilogue) can reach, in units of
    o["unit"], the smallest unit in use: must stay below 2^24"""
    m = lin(c, o["w"].abs(), o["x"].abs()) + o["bias"].abs().view(1, -1, 1)
    top = float(m.max())
    if c.act is None:
        for k in EP:
            if k not in c.ep:
                continue
            if k == "ch_scale":
                m = m * per_row(c, o[k]).abs()
            else:
                m = m + (per_row(c, o[k]) if k == "post_add" else o[k]).abs()
            top = max(top, float(m.max()))
    return top / o["unit"]


def lerp_coord(t, ratio, lf):
    """csrc/common.h::lerp_coord for integer columns t (NumPy): src = fmaf(ratio, t + 0.5, -0.5) clamped at 0 in fp32 (the float64
    product of two fp32 numbers is exact, so one rounding like the fma), i0 = int(src) clamped, i1 = i0 + 1 clamped"""
    src = (np.float64(np.float32(ratio)) * (np.asarray(t, np.float64) + 0.5) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0.0))
    i0 = np.minimum(src.astype(np.int64), lf - 1)
    i1 = i0 + (i0 < lf - 1)
    return i0, i1


def first_diff(a, b, bad=None):
    """(n, row, t), a's and b's value at the first element where a != b (or where `bad` is set); None if there is none"""
    bad = (a != b) if bad is None else bad
    if not bool(bad.any()):
        return None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return idx, float(a[idx]), float(b[idx])


# -------------------------------------------------------------------------------------------------------------- the matrix ----
def _act_wa(K, xa=3):
    """weights w = iw 2^-6: |iw| <= wa chosen for std(v) of about 2.5, so that v covers multiples of 1/64 in about +-8"""
    sx = math.sqrt(xa * (xa + 1) / 3.0)
    return max(1, min(127, round(math.sqrt(3.0) * 2.5 * 64.0 / (sx * math.sqrt(K)))))


def _with_act(c, act):
    return replace(c, act=act, wexp=-6, wa=_act_wa(c.K, c.xa))


def exact_cases():
    E = lambda **k: Case(kernel="exact", prec="fp32", **k)
    out = []
    for co in (1, 16, 17, 64, 65, 129):                                            # 16-, 64- and 128-row tiles, ragged last tile
        out.append(E(tag="rows", n=2, ci=5, co=co, kw=3, tin=100))
    for tout in (97, 128, 129, 256, 257):                                          # K = 15 padded to 16; column tile edges
        out.append(E(tag="kpad", n=2, ci=5, co=17, kw=3, tin=tout + 2))
    for kw, s in ((2, 2), (8, 8), (10, 10), (7, 3)):
        out.append(E(tag="stride", n=1, ci=6, co=20, kw=kw, stride=s, tin=129 * s + kw))
    out.append(E(tag="ci1", n=1, ci=1, co=8, kw=40, stride=10, tin=129 * 10 + 40))  # kw_magic == 0
    out.append(E(tag="ci1", n=1, ci=1, co=8, kw=40, stride=10, pad=20, mode=2, tin=1000, out_len=101))
    out.append(E(tag="zeropad", n=1, ci=4, co=8, kw=7, pad=3, tin=120, out_len=130))
    out.append(E(tag="reflL", n=1, ci=4, co=20, kw=5, pad=59, mode=1, tin=60))
    out.append(E(tag="reflLR", n=1, ci=4, co=20, kw=7, pad=3, mode=2, tin=128, out_len=128))
    out.append(E(tag="wrap", n=1, ci=4100, co=8, kw=2, stride=2, tin=194, xa=1, wa=1, hot=4096))
    out.append(E(tag="wrap", n=1, ci=4100, co=8, kw=5, tin=101, xa=1, wa=1, hot=4096))
    for co, r in ((8, 2), (4, 4), (3, 4), (7, 2)):                                 # vector-store kernel; ragged rows
        out.append(E(tag="upv", n=2, ci=8, co=co, r=r, tin=100))
        out.append(E(tag="upv", n=2, ci=8, co=co, r=r, tin=100, ep=("post_add",)))
    out.append(E(tag="up", n=2, ci=8, co=20, r=10, tin=100))
    out.append(E(tag="up", n=2, ci=8, co=20, r=10, tin=100, ep=("post_add", "ch_scale")))
    for co in (20, 64):
        for yp in (1, 2):
            out.append(E(tag="yp", n=3, ci=6, co=co, kw=2, stride=2, tin=86, yp=yp))
    for co in (16, 40, 80):
        base = E(tag="ep", n=2, ci=8, co=co, kw=3, tin=70)
        out += [replace(base, ep=ep) for ep in EP_SUBSETS if ep]
        out += [_with_act(replace(base, tag="act"), a) for a in ("gelu", "exp", "sin")]
        out.append(_with_act(replace(base, tag="act", ep=("post_add", "ch_scale", "residual")), "gelu"))
        out.append(replace(base, tag="film", tin=132, lf=13, want_raw=False, wexp=-6, wa=_act_wa(24)))
        out.append(replace(base, tag="film", tin=132, lf=200, ep=("residual",), wexp=-6, wa=_act_wa(24)))
    for lf in (13, 130, 200, 1):                                                    # LDS slab; global fallback (lf >= tout); one frame
        out.append(E(tag="film", n=2, ci=8, co=40, kw=3, tin=132, lf=lf, wexp=-6, wa=_act_wa(24)))
    return out


SPLIT_COMBOS = [("bf16x3", "I"), ("bf16x3", "IIw"), ("bf16x3", "IIx"), ("bf16x3", "IIwx"), ("bf16x6", "I"), ("bf16x6", "IIw"),
                ("bf16x6", "IIx"), ("fp16", "I")]
# (co, ci, kw, dil, pad, mode, tout): the tile rows, the tail channel block, the halo limit (kw - 1) dil = 16, both epilogues
SPLIT_SHAPES = [(40, 24, 5, 4, 16, 1, 100), (64, 32, 3, 8, 16, 1, 128), (65, 33, 8, 2, 3, 0, 129), (129, 96, 1, 1, 0, 0, 130),
                (192, 33, 5, 4, 0, 1, 256), (129, 24, 3, 8, 3, 1, 100), (40, 96, 8, 2, 16, 0, 130), (192, 32, 1, 1, 0, 0, 129)]


def split_cases():
    out = []
    S = lambda **k: Case(kernel="split", **k)
    for prec, reg in SPLIT_COMBOS:
        for co, ci, kw, dil, pad, mode, tout in SPLIT_SHAPES:
            out.append(S(tag="shape", prec=prec, regime=reg, n=2, ci=ci, co=co, kw=kw, dil=dil, pad=pad, mode=mode,
                         tin=tout - pad + dil * (kw - 1), xa=2))
    for co, tin in ((40, 130), (129, 128), (129, 129)):                            # scalar (Tout % 4 != 0) and vector epilogue
        for prec, reg in (("bf16x3", "I"), ("bf16x6", "IIw"), ("fp16", "I")):
            base = S(tag="ep", prec=prec, regime=reg, n=2, ci=24, co=co, kw=3, pad=2, mode=1, tin=tin)
            eps = EP_SUBSETS if prec == "bf16x3" else [EP, ("ch_scale", "skip")]
            out += [replace(base, ep=ep) for ep in eps if ep]
        base = S(tag="act", prec="bf16x3", n=2, ci=24, co=co, kw=3, pad=2, mode=1, tin=tin)
        out += [_with_act(base, a) for a in ("gelu", "exp")]
        out.append(_with_act(replace(base, ep=("post_add", "ch_scale", "residual", "skip")), "gelu"))
        out.append(_with_act(replace(base, prec="fp16"), "gelu"))
    fw = dict(wexp=-6, wa=_act_wa(72))
    for prec in ("bf16x3", "fp16"):
        base = S(tag="film", prec=prec, n=2, ci=24, co=129, kw=3, pad=2, mode=1, tin=100, **fw)
        out.append(replace(base, tin=130, lf=13))                                   # scalar epilogue (Tout % 4 != 0) + FiLM
        out.append(replace(base, tin=130, lf=13, want_raw=False, ep=("residual",)))
        out.append(replace(base, tin=129, lf=13, co=40))
        out.append(replace(base, tin=120, lf=12))                                   # vector epilogue + FiLM
        out.append(replace(base, tin=120, lf=12, want_raw=False, co=40))
        out.append(replace(base, tin=128, lf=17))                                   # the largest admitted span: 17 / 128 * 128 + 3 = 20
        out.append(replace(base, tin=130, lf=17, co=64))                            # (scalar: 19.7)
        out.append(replace(base, tin=130, lf=1))
        out.append(replace(base, tin=120, lf=2))
    out.append(_with_act(S(tag="film", prec="bf16x3", n=2, ci=24, co=65, kw=3, pad=2, mode=1, tin=130, lf=13), "gelu"))
    for prec, reg in (("bf16x3", "I"), ("bf16x3", "IIx"), ("bf16x3", "IIwx"), ("fp16", "I")):
        for co, ci, kw, dil, pad, tin in ((128, 32, 5, 2, 8, 128), (192, 64, 1, 1, 0, 132), (192, 32, 5, 4, 16, 260)):
            base = S(tag="planes", prec=prec, regime=reg, n=2, ci=ci, co=co, kw=kw, dil=dil, pad=pad, mode=1, tin=tin, xa=2)
            out.append(replace(base, xp=True))
            if reg == "I":
                out.append(replace(base, zp=True, lf=tin // 10, **fw))
                out.append(replace(base, xp=True, zp=True, lf=tin // 10, want_raw=False, ep=("residual",), **fw))
    ups = [(10, 4), (9, 8), (5, 16), (3, 64),                                      # power-of-two vector path
           (33, 2), (43, 3), (13, 10)]                                             # general path: channels straddle rows 64 and 128
    for co, r in ups:
        for prec, reg in (("bf16x3", "I"), ("bf16x3", "IIwx"), ("bf16x6", "IIw"), ("fp16", "I")):
            if prec != "bf16x3" and r not in (16, 3, 10):
                continue
            out.append(S(tag="up", prec=prec, regime=reg, n=2, ci=24, co=co, r=r, tin=100, xa=2))
        out.append(_with_act(S(tag="up", prec="bf16x3", n=2, ci=24, co=co, r=r, tin=100, ep=("post_add", "ch_scale")), "gelu"))
        out.append(S(tag="up", prec="bf16x3", n=2, ci=24, co=co, r=r, tin=100, ep=("post_add", "ch_scale")))
    return out


SKINNY_COMBOS = [("fp32", "I"), ("bf16x3", "I"), ("bf16x6", "I"), ("fp32", "IIw"), ("bf16x3", "IIx"), ("bf16x6", "IIw"),
                 ("fp32", "IIx"), ("bf16x3", "IIw"), ("bf16x6", "IIx")]
SKINNY_COLUMNS = [(1, 1), (1, 15), (1, 16), (1, 17), (3, 7), (1, 33), (5, 19), (96, 1), (1, 96)]


def skinny_cases():
    out = []
    K = lambda **k: Case(kernel="skinny", **k)
    for i, (n, tout) in enumerate(SKINNY_COLUMNS):                                  # batch boundaries inside a 16-column tile
        for q in range(3):
            prec = ("fp32", "bf16x3", "bf16x6")[q]
            reg = ("I", "IIw", "IIx")[(i + q) % 3]
            out.append(K(tag="cols", prec=prec, regime=reg, n=n, ci=20, co=17, kw=3, pad=1, tin=tout, out_len=tout, xa=2))
    for prec, reg in SKINNY_COMBOS:
        for co in (1, 17, 40):
            out.append(K(tag="rows", prec=prec, regime=reg, n=3, ci=33, co=co, kw=1, tin=7, xa=2))
        # the 8- / 16-wave switch at a padded K of 512: K_pad 496 | 512 (fp32 rows), KW * Ci_pad 480 | 512 (planes)
        for ci, kw in (((31, 16), (32, 16)) if prec == "fp32" else ((30, 15), (32, 16))):
            out.append(K(tag="kswitch", prec=prec, regime=reg, n=2, ci=ci, co=17, kw=kw, tin=kw + 5, xa=2))
        # pointwise, and the three ways out of the pointwise path
        out.append(K(tag="pw", prec=prec, regime=reg, n=3, ci=40, co=17, tin=7, xa=2))
        out.append(K(tag="pw-pad", prec=prec, regime=reg, n=3, ci=40, co=17, pad=2, tin=7, xa=2))
        out.append(K(tag="pw-stride", prec=prec, regime=reg, n=3, ci=40, co=17, stride=2, tin=14, xa=2))
        out.append(K(tag="pw-long", prec=prec, regime=reg, n=3, ci=40, co=17, tin=7, out_len=9, xa=2))
        out.append(K(tag="geo", prec=prec, regime=reg, n=2, ci=33, co=17, kw=5, dil=4, pad=16, mode=1, tin=19, xa=2))
        out.append(K(tag="geo", prec=prec, regime=reg, n=2, ci=33, co=17, kw=8, stride=8, tin=8 * 11, xa=2))
        out.append(K(tag="geo", prec=prec, regime=reg, n=2, ci=33, co=17, kw=5, stride=2, pad=3, mode=2, tin=30, out_len=17, xa=2))
        out.append(K(tag="geo", prec=prec, regime=reg, n=2, ci=33, co=17, kw=5, dil=2, pad=3, mode=0, tin=20, out_len=23, xa=2))
        for co, r in ((9, 2), (5, 10)):
            out.append(K(tag="up", prec=prec, regime=reg, n=2, ci=33, co=co, r=r, tin=21, xa=2))
    for i, ep in enumerate(e for e in EP_SUBSETS if e):
        prec, reg = SKINNY_COMBOS[i % 9]
        out.append(K(tag="ep", prec=prec, regime=reg, n=3, ci=33, co=17, kw=3, pad=2, mode=1, tin=19, ep=ep, xa=2))
    for prec in ("fp32", "bf16x3", "bf16x6"):
        base = K(tag="act", prec=prec, n=3, ci=33, co=17, kw=3, pad=2, mode=1, tin=19)
        out += [_with_act(base, a) for a in ("gelu", "exp", "sin")]
        out.append(_with_act(replace(base, ep=EP), "gelu"))
        for lf in (5, 19, 40):                                                      # Lf < Tout, = Tout, > Tout
            out.append(replace(base, tag="film", lf=lf, wexp=-6, wa=_act_wa(99), want_raw=lf != 19))
    return out


def seam_cases():
    """pairs (96 columns: few-column kernel; 97: a batch kernel) of one conv with the same input: the 96 shared columns must be
    bitwise equal to each other and to the reference"""
    geo = [dict(prec="fp32", ci=40, co=17), dict(prec="bf16x3", regime="IIw", ci=40, co=17, xa=2),
           dict(prec="bf16x6", regime="IIx", ci=64, co=80, xa=2),
           dict(prec="bf16x3", regime="IIx", ci=33, co=40, kw=5, dil=4, pad=16, mode=1, xa=2),
           dict(prec="fp32", ci=6, co=20, kw=4, stride=3),
           dict(prec="fp32", ci=4100, co=8, kw=2, stride=2, xa=1, wa=1, hot=4096)]
    out = []
    for g in geo:
        kw, s, dil, pad = g.get("kw", 1), g.get("stride", 1), g.get("dil", 1), g.get("pad", 0)
        tin = 96 * s + dil * (kw - 1) + 1 - pad                                    # 97 natural columns
        big = "exact" if g["prec"] == "fp32" else "split"
        out.append((Case(kernel="skinny", tag="seam", n=1, tin=tin, out_len=96, **g), Case(kernel=big, tag="seam", n=1, tin=tin, out_len=97, **g)))
    return out


# ---- Gaussian operands for what stays on a tolerance: the third plane of bf16x6, bf16x6 with both operands split, fp16 off the grid ----
TOL_SHAPE = dict(n=2, ci=33, co=129, kw=5, dil=2, pad=8, mode=1, tin=130)


def split_planes(t, planes):
    """fp32 -> the bf16 planes the kernels form (round to nearest each step), as float64"""
    out, r = [], t.float()
    for _ in range(planes):
        h = r.bfloat16().float()
        out.append(h.double())
        r = r - h
    return out


def tolerance_case(prec):
    """Gaussian x, w, bias; -> (case, operands, ref, bound): ref = the float64 conv of the operands as the kernel decodes them (sum of
    its planes, or the fp16 value), bound per element = (K + 4) 2^-24 (sum |w| |x| + |b|), the first-order worst case of an fp32
    accumulation, plus the plane products the precision drops (every pair with i + j >= planes), exactly from the planes"""
    c = Case(kernel="split", prec=prec, tag="gauss", **TOL_SHAPE)
    rng = np.random.default_rng(c.seed)
    x = torch.from_numpy(rng.standard_normal((c.n, c.ci, c.tin))).float()
    w = torch.from_numpy(rng.standard_normal((c.co, c.ci, c.kw)) / math.sqrt(c.K)).float()
    b = torch.from_numpy(rng.standard_normal((c.co,)) * 0.1).float()
    if prec == "fp16":
        wd, xd = w.half().double(), x.half().double()
        dropped = torch.zeros(())
    else:
        P = NPLANES[prec]
        wp, xp = split_planes(w, P), split_planes(x, P)
        wd, xd = sum(wp), sum(xp)
        dropped = sum(lin(c, wp[i], xp[j]).abs() for i in range(P) for j in range(P) if i + j >= P)
    ref = lin(c, wd, xd) + b.double().view(1, -1, 1)
    mag = lin(c, wd.abs(), xd.abs()) + b.double().abs().view(1, -1, 1)
    bound = (c.K + 4) * 2.0 ** -24 * mag + dropped
    return c, {"x": x, "w": w, "bias": b}, ref, bound


def all_exact_operand_cases():
    seams = [c for pair in seam_cases() for c in pair]
    return exact_cases() + split_cases() + skinny_cases() + seams
