"""Operands, references and the case matrix of the exact-operand tests of alive_gemm_planes (csrc/gemm_planes.hip).  NumPy and torch on
the CPU only; the library is not imported here.  tests/test_host_gemm_operands.py proves on the CPU what the generators promise,
tests/test_gpu_gemm_exact.py runs the matrix on the device.  The pattern, the activation bounds and first_diff are tests/conv_cases.py's.

Every operand is a sum of up to three PLANES (the kernel's own decomposition: bf16 round-to-nearest remainders, or the fp16 (hi, lo) pair
of a power-of-two multiple), designed so that every product of two planes the kernel keeps, and every partial sum of such products in any
order, is an fp32 number: the result then does not depend on tile shape, k-step depth, ring depth, MFMA order or persistence, the
tolerance is zero and a mismatch names an element (n, row, t).  The expected value is the sum over the KEPT plane pairs (i + j <= NP - 1)
and nothing else -- not the true product where the kernel drops a pair.

  "I"      small integers times a power of two; every lo plane is zero.  Every form.
  "IIw"    w = a + b 2^-10 (a in +-{1, 2}, b = sign(a) {0 .. 3}): planes (a, b 2^-10, 0); x integer.  "IIx": the roles exchanged;
           "IIwx": both.  Two planes keep (0,0) (0,1) (1,0) and drop (1,1); three planes keep all four (dense: K <= 3 only).
  "IIIw"   w = a + b 2^-10 + c 2^-20 (b = sign(a) {1 .. 3}, c = sign(a) {0 .. 3}): three real planes.  A dense product of such values
           needs 29 bits, so x is an integer SPARSE along K: up to five +-1 per column, one per k-block, walking through the 32 k of
           a block from column to column.  "IIIx": the roles exchanged (sparse rows of w).
  "III11"  w as in IIw, x = a + b 2^-10 (b != 0) sparse along K: the pair (1, 1) is non-zero and kept (three planes).
  "III21"  w as in IIIw, x as in III11: the pair (2, 1) is non-zero (units of 2^-30) and dropped.
  "Fw"     f16s: w = a + b 2^-13 (b = sign(a) {0, 1}, one |a| = 2, so that pack_conv_split_f16s picks the scale 2^12):
           images hi = 4096 a, lo = b / 2; x integer.  "Fx": x = a / 16 + b 2^-16: images hi = 16 a, lo = b 2^-8 of 2^8 x.  "Fwx": both.
  "Hw"     one fp16 plane: w = +-(1 + j 2^-10), 11 significant bits; x integer.  "Hx": the roles exchanged.
In every regime |bias| + sum |w| |x| and what the epilogue adds stay below 2^24 of the smallest unit in use (checked on the CPU).

Behind an activation v is still exact and the only error left is the function's own (bounds of conv_cases.py, derived there from the
definitions: gelu_fast 4e-7 |v| + 2^-22 |gelu(v)|, expf 2^-21 max(|v|, |f(v)|), 2^-24 of its result per add of the linear tail)."""
import itertools
import math
import os
import sys
import zlib
from dataclasses import dataclass, replace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_cases import _act_wa, _ints, _split_vals, first_diff, gelu64, pad32, tol_gelu_fast  # noqa: E402,F401

GM = GN = 128                     # tile
GK = 32                           # k per step (the 64-deep form: two of them)
PERSIST_TILES, PERSIST_STEPS = 512, 3
KB2_MIN = 128                     # planes 1: pad32(Ci) % 64 == 0 and >= 128 -> the 64-deep step
RING = {"np1": 4, "kb2": 2, "np2": 2, "f16s": 2, "np3": 3, "np3lw": 3}
PLANES = {"np1": 1, "kb2": 1, "np2": 2, "f16s": 2, "np3": 3, "np3lw": 3}
ACTS = {None: 0, "gelu": 1, "exp": 2, "argmax": 3}
EP = ("bias", "post_add", "ch_scale", "residual")
EP_SUBSETS = [tuple(e for e, on in zip(EP, bits) if on) for bits in itertools.product((0, 1), repeat=4)]
F16S_ACT_SCALE = 256.0            # the multiple of the fp16 split activations (csrc/networks.hip)
SPLIT_REGIMES = ("IIw", "IIx", "IIwx", "IIIw", "IIIx", "III11", "III21", "Fw", "Fx", "Fwx")
CO_EDGES = (1, 5, 17, 33, 63, 64, 65, 127, 128, 129, 200)
CI_EDGES = (1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129)


def cdiv(a, b):
    return (a + b - 1) // b


@dataclass(frozen=True)
class Case:
    form: str                 # the instantiation alive_gemm_planes must reach: a key of RING
    n: int
    t: int
    ci: int
    co: int
    act: str = None           # None | "gelu" | "exp" | "argmax"
    ep: tuple = ("bias",)
    alias: bool = False       # Y is the residual tensor
    out: str = "y"            # "y" | "p" | "yp"; argmax: "a"
    regime: str = "I"
    xa: int = 2
    wa: int = 2
    wexp: int = 0
    tag: str = ""

    @property
    def planes(self):
        return PLANES[self.form]

    @property
    def f16s(self):
        return self.form == "f16s"

    @property
    def cols(self):
        return self.n * self.t

    @property
    def cols_pad(self):
        return cdiv(self.cols, GN) * GN

    @property
    def nsteps(self):
        return pad32(self.ci) // (2 * GK if self.form == "kb2" else GK)

    @property
    def ntiles(self):
        return cdiv(self.co, GM) * cdiv(self.cols, GN)

    @property
    def np_(self):
        """planes of the product rule: pairs (i, j) with i + j <= np_ - 1"""
        return self.planes

    @property
    def id(self):
        s = f"{self.tag}-{self.form}-{self.regime}-n{self.n}t{self.t}ci{self.ci}co{self.co}-{self.out}"
        if self.ep != ("bias",):
            s += "-" + ("+".join(e[:2] for e in self.ep) or "none")
        if self.alias:
            s += "-alias"
        if self.act:
            s += "-" + self.act
        return s

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())


def dispatch(planes, f16s, n, t, ci, co):
    """the form alive_gemm_planes chooses (ALIVE_GEMM_VARIANT unset, standard row walk), restated from its dispatch"""
    if planes == 1:
        return "kb2" if pad32(ci) % 64 == 0 and pad32(ci) >= KB2_MIN else "np1"
    if planes == 2:
        return "f16s" if f16s else "np2"
    ntiles, nsteps = cdiv(co, GM) * cdiv(n * t, GN), pad32(ci) // GK
    return "np3lw" if ntiles >= PERSIST_TILES and nsteps >= PERSIST_STEPS else "np3"


def dispatch_case(c):
    return dispatch(c.planes, c.f16s, c.n, c.t, c.ci, c.co)


def kept_pairs(c):
    return [(i, j) for i in range(3) for j in range(3) if i + j <= c.np_ - 1]


def dropped_pairs(c):
    return [(i, j) for i in range(3) for j in range(3) if i + j > c.np_ - 1]


# ---------------------------------------------------------------------------------------------------------------- operands ----
def sparse_mask(rows, ci, m):
    """[rows][ci] bool: row r holds entries in the k-blocks (r + i) % nkb, i < m, at offset (7 r + 11 i) % width inside the block:
    with m >= nkb every row reaches every k-block, and the offsets walk through a block from row to row"""
    nkb = cdiv(ci, GK)
    r = np.arange(rows).reshape(-1, 1)
    i = np.arange(m).reshape(1, -1)
    blk = (r + i) % nkb
    width = np.minimum(GK, ci - blk * GK)
    k = blk * GK + (7 * r + 11 * i) % width
    M = np.zeros((rows, ci), dtype=bool)
    M[np.broadcast_to(r, k.shape), k] = True
    return torch.from_numpy(M)


def _zeros(shape):
    return torch.zeros(shape, dtype=torch.float64)


def _three(rng, shape):
    """a + b 2^-10 + c 2^-20, b = sign(a) {1 .. 3}, c = sign(a) {0 .. 3}: bf16 planes (a, b 2^-10, c 2^-20).  (b = 0 would move c up
    into the second plane; c = 4 at b = 1 would tie at half an ulp of 2^-10's bf16.)"""
    a = torch.from_numpy(rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=shape))
    b = torch.from_numpy(rng.integers(1, 4, size=shape)).double() * a.sign()
    c = torch.from_numpy(rng.integers(0, 4, size=shape)).double() * a.sign()
    return [a, b * 2.0 ** -10, c * 2.0 ** -20]


def _two(rng, shape):
    a, b = _split_vals(rng, shape)
    return [a, b * 2.0 ** -10, _zeros(shape)]


def _f16pair(rng, shape, hi_unit, lo_unit):
    a = torch.from_numpy(rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=shape))
    b = torch.from_numpy(rng.integers(0, 2, size=shape)).double() * a.sign()
    return [a * hi_unit, b * lo_unit, _zeros(shape)]


def _h11(rng, shape):
    s = torch.from_numpy(rng.choice(np.array([-1.0, 1.0]), size=shape))
    return [s * (1.0 + torch.from_numpy(rng.integers(0, 1024, size=shape)).double() * 2.0 ** -10), _zeros(shape), _zeros(shape)]


def _int_planes(rng, shape, a, u=1.0):
    return [_ints(rng, shape, a) * u, _zeros(shape), _zeros(shape)]


def _nz_int_planes(rng, shape, a):
    """+-{1 .. a}: the integer partner of a split operand has no zeros, so that no lo plane of the other side goes unseen behind one"""
    v = torch.from_numpy(rng.integers(1, a + 1, size=shape) * rng.choice(np.array([-1, 1]), size=shape)).double()
    return [v, _zeros(shape), _zeros(shape)]


def _sparse_m(c):
    """entries per sparse row: one per k-block (at least 3); the budget of the regime caps it (asserted in the matrix test)"""
    return max(3, cdiv(c.ci, GK))


def make(c):
    """the case's operands as float64 CPU tensors (each an fp32 number): x [n][ci][t] and its planes xp[0..2], w [co][ci] and wp[0..2],
    bias [co], post_add / ch_scale [co], residual [n][co][t].  `unit`: every value up to the activation is a multiple of it."""
    rng = np.random.default_rng(c.seed)
    wshape, xshape = (c.co, c.ci), (c.n, c.ci, c.t)
    u = 2.0 ** c.wexp
    R = c.regime
    x_mask = lambda: sparse_mask(c.cols, c.ci, _sparse_m(c)).view(c.n, c.t, c.ci).permute(0, 2, 1).double()
    w_mask = lambda: sparse_mask(c.co, c.ci, _sparse_m(c)).double()
    pm1 = lambda shape: torch.from_numpy(rng.choice(np.array([-1.0, 1.0]), size=shape))
    if R == "I":
        wp, xp, unit = _int_planes(rng, wshape, c.wa, u), _int_planes(rng, xshape, c.xa), u
    elif R in ("IIw", "IIx", "IIwx"):
        wp = _two(rng, wshape) if "w" in R else _nz_int_planes(rng, wshape, c.wa)
        xp = _two(rng, xshape) if "x" in R else _nz_int_planes(rng, xshape, c.xa)
        unit = 2.0 ** -20 if (R == "IIwx" and c.np_ == 3) else 2.0 ** -10
    elif R == "IIIw":
        wp, m = _three(rng, wshape), x_mask()
        xp, unit = [pm1(xshape) * m, _zeros(xshape), _zeros(xshape)], 2.0 ** -20
    elif R == "IIIx":
        xp, m = _three(rng, xshape), w_mask()
        wp, unit = [pm1(wshape) * m, _zeros(wshape), _zeros(wshape)], 2.0 ** -20
    elif R in ("III11", "III21"):
        wp, m = (_two if R == "III11" else _three)(rng, wshape), x_mask()
        xp, unit = [p * m for p in _three(rng, xshape)[:2]] + [_zeros(xshape)], 2.0 ** -20       # (b != 0: a lo plane in every entry)
    elif R in ("Fw", "Fx", "Fwx"):
        wp = _f16pair(rng, wshape, 1.0, 2.0 ** -13) if "w" in R else _nz_int_planes(rng, wshape, c.wa)
        xp = _f16pair(rng, xshape, 2.0 ** -4, 2.0 ** -16) if "x" in R else _nz_int_planes(rng, xshape, c.xa)
        if "w" in R:
            wp[0][0, 0] = math.copysign(2.0, float(wp[0][0, 0]))                  # max |w| in (2, 4): the packer's scale is 2^12
        unit = {"Fw": 2.0 ** -13, "Fx": 2.0 ** -16, "Fwx": 2.0 ** -17}[R]
    elif R in ("Hw", "Hx"):
        wp = _h11(rng, wshape) if R == "Hw" else _int_planes(rng, wshape, c.wa)
        xp = _h11(rng, xshape) if R == "Hx" else _int_planes(rng, xshape, c.xa)
        unit = 2.0 ** -10
    else:
        raise ValueError(R)
    bu = u if R == "I" else 1.0
    o = {"bias": _ints(rng, (c.co,), 4 if R == "I" else 2) * bu if "bias" in c.ep else None}
    if "post_add" in c.ep:
        o["post_add"] = _ints(rng, (c.co,), 3) * bu
    if "ch_scale" in c.ep:
        e = rng.integers(-1 if R == "I" else 0, 2, size=(c.co,))
        o["ch_scale"] = torch.from_numpy(rng.choice(np.array([-1.0, 1.0]), size=(c.co,)) * 2.0 ** e)
        if R == "I":
            unit = unit / 2.0
    if "residual" in c.ep:
        o["residual"] = _ints(rng, (c.n, c.co, c.t), 8) * bu
    if c.act == "argmax" and c.tag != "narrow":
        # twins: rows [h, co) repeat rows [0, co - h), h a multiple of 64 -> every such pair ties ACROSS 64-row blocks; every third
        # twin gets a bias one higher, so that the first maximum also falls into the upper rows
        h = twin_offset(c.co)
        for p in wp:
            p[h:] = p[:c.co - h]
        if o["bias"] is not None:
            o["bias"][h:] = o["bias"][:c.co - h]
            o["bias"][h::3] += bu
    o.update(wp=wp, xp=xp, w=wp[0] + wp[1] + wp[2], x=xp[0] + xp[1] + xp[2], unit=unit)
    return o


def twin_offset(co):
    return cdiv(cdiv(co, 2), 64) * 64


# -------------------------------------------------------------------------------------------------------------- references ----
def lin(w, x, ks=None):
    """[co][ci] x [n][ci][t] -> [n][co][t] in float64 (exact: every operand here has at most 22 bits); ks: a slice of k"""
    if ks is not None:
        w, x = w[:, ks], x[:, ks]
    return torch.matmul(w, x)


def pair_sum(c, o, pairs, ks=None):
    tot = _zeros((c.n, c.co, c.t))
    for i, j in pairs:
        if bool(o["wp"][i].any()) and bool(o["xp"][j].any()):
            tot = tot + lin(o["wp"][i], o["xp"][j], ks)
    return tot


def value(c, o, pairs=None):
    """v before the activation, exact in float64: the kept plane pairs (or `pairs`) + bias"""
    v = pair_sum(c, o, kept_pairs(c) if pairs is None else pairs)
    return v if o["bias"] is None else v + o["bias"].view(1, -1, 1)


def reference(c, o):
    """{"v", "y", "yerr"}: float64; yerr == 0 everywhere <=> the output is exact and compared bit for bit.
    Order of gemm_epilogue: act, (+ post_add) * ch_scale, + residual."""
    v = value(c, o)
    if c.act in (None, "argmax"):
        y, err = v, torch.zeros_like(v)
    elif c.act == "gelu":
        y, err = gelu64(v), tol_gelu_fast(v)
    else:
        y = torch.exp(v)
        err = 2.0 ** -21 * torch.maximum(v.abs(), y.abs())
    for k in EP[1:]:
        if k not in c.ep:
            continue
        if k == "ch_scale":
            s = o[k].view(1, -1, 1)
            y, err = y * s, err * s.abs()
        else:
            y = y + (o[k].view(1, -1, 1) if k == "post_add" else o[k])
            if c.act is not None:
                err = err + 2.0 ** -24 * y.abs()
    return {"v": v, "y": y, "yerr": err}


def unit_sum_bound(c, o):
    """the largest magnitude any partial sum of plane products (every plane of an operand has the operand's sign, so |w| |x| bounds
    every subset of pairs) and, without an activation, any stage of the epilogue can reach, in units of o["unit"]: below 2^24"""
    m = lin(o["w"].abs(), o["x"].abs())
    if o["bias"] is not None:
        m = m + o["bias"].abs().view(1, -1, 1)
    top = float(m.max())
    if c.act is None:
        for k in EP[1:]:
            if k not in c.ep:
                continue
            if k == "ch_scale":
                m = m * o[k].abs().view(1, -1, 1)
            else:
                m = m + (o[k].view(1, -1, 1) if k == "post_add" else o[k]).abs()
            top = max(top, float(m.max()))
    return top / o["unit"]


def argmax_reference(c, v):
    """(val [blocks][cols], idx [blocks][cols], first index of the maximum [cols], share of the columns whose maximum is reached in
    more than one 64-row block) of the exact values v [n][co][t]"""
    a = v.permute(1, 0, 2).reshape(c.co, c.cols).numpy()
    nblk = cdiv(c.co, 64)
    val, idx = np.empty((nblk, c.cols)), np.empty((nblk, c.cols), dtype=np.int64)
    for b in range(nblk):
        blk = a[64 * b:64 * b + 64]
        idx[b] = blk.argmax(0) + 64 * b                                        # NumPy: the first occurrence
        val[b] = blk.max(0)
    first = a.argmax(0)
    ties = float(((val == a.max(0, keepdims=True)).sum(0) > 1).mean())
    return val, idx, first, ties


# ---------------------------------------------------------------------------------------------------------- the host codec ----
def host_planes(x, kind, scale=1.0):
    """fp32-valued [n][c][t] -> the k-blocked plane image int16 [planes][c_pad / 32][cols_pad][32] (csrc/planes_layout.h), zero
    padded: kind 1 = one fp16 plane, 2 / 3 = bf16 round-to-nearest-even remainders, "f16s" = fp16 (hi, lo) of scale * x"""
    n, ch, t = x.shape
    cols, cp = n * t, pad32(ch)
    cols_pad = cdiv(cols, GN) * GN
    flat = torch.zeros(cols_pad, cp, dtype=torch.float32)
    flat[:cols, :ch] = x.float().permute(0, 2, 1).reshape(cols, ch)
    if kind == 1:
        pl = [flat.clamp(-65504.0, 65504.0).half().view(torch.int16)]
    elif kind == "f16s":
        q = flat * scale
        hi = q.clamp(-65504.0, 65504.0).half()
        lo = (q - hi.float()).clamp(-65504.0, 65504.0).half()
        pl = [hi.view(torch.int16), lo.view(torch.int16)]
    else:
        pl, r = [], flat
        for _ in range(kind):
            h = r.bfloat16()
            pl.append(h.view(torch.int16))
            r = r - h.float()
    return torch.stack(pl, 0).view(len(pl), cols_pad, cp // 32, 32).permute(0, 2, 1, 3).contiguous()


def plane_kind(c):
    return "f16s" if c.f16s else c.planes


def planes_as_float(P, c):
    """int16 plane image -> float64 values of its elements (bf16, or fp16 for one plane / f16s)"""
    return (P.view(torch.float16) if (c.f16s or c.planes == 1) else P.view(torch.bfloat16)).double()


def tiles_any(c, d):
    """[row tiles][column tiles] bool: some element of the tile is set in d [n][co][t]"""
    a = torch.zeros(cdiv(c.co, GM) * GM, c.cols_pad, dtype=torch.bool)
    a[:c.co, :c.cols] = d.permute(1, 0, 2).reshape(c.co, c.cols)
    return a.view(cdiv(c.co, GM), GM, c.cols_pad // GN, GN).any(3).any(1)


# -------------------------------------------------------------------------------------------------------------- the matrix ----
def _with_act(c, act, K=None):
    """regime I: w = iw 2^-6 with std(v) of about 2.5 (conv_cases._act_wa); the split regimes of f16s reach that range by themselves"""
    if c.regime != "I":
        return replace(c, act=act)
    return replace(c, act=act, wexp=-6, wa=_act_wa(c.ci, c.xa))


def step_cases():
    """every form at each required depth of its DMA ring: fewer steps than the ring, as many, more"""
    out = []
    for i, ci in enumerate((20, 64, 96, 129)):                                              # 1, 2, 3, 5 steps, ring of 4
        out.append(Case("np1", tag="steps", n=1, t=130, ci=ci, co=137, regime=("I", "Hw", "Hx", "I")[i], out=("y", "yp", "p", "yp")[i]))
    for ci in (128, 161, 256):                                                               # 2, 3, 4 steps of 64
        for j, act in enumerate((None, "gelu", "exp")):
            base = Case("kb2", tag="steps", n=1, t=130, ci=ci, co=137, regime=("Hw", "I", "I")[j], out=("yp", "yp", "y")[j])
            out.append(_with_act(base, act) if act else base)
    for i, ci in enumerate((31, 33, 65, 129)):                                               # 1, 2, 3, 5 steps, ring of 2
        out.append(Case("np2", tag="steps", n=1, t=130, ci=ci, co=137, regime=("IIwx", "IIw", "IIx", "IIwx")[i], out=("yp", "y", "p", "yp")[i]))
    for i, ci in enumerate((32, 64, 97, 160)):
        out.append(Case("f16s", tag="steps", n=1, t=130, ci=ci, co=137, regime=("Fwx", "Fw", "Fx", "Fwx")[i], xa=1, out=("yp", "y", "p", "yp")[i]))
    for i, (ci, reg) in enumerate(((1, "IIw"), (3, "IIwx"), (63, "IIIw"), (96, "IIIx"), (128, "IIIw"), (96, "III11"), (96, "III21"), (128, "IIx"))):
        out.append(Case("np3", tag="steps", n=1, t=130, ci=ci, co=137, regime=reg, out=("yp", "y", "p")[i % 3]))    # 1, 1, 2, 3, 4, 3, 3, 4 steps
    return out


def act_cases():
    out = []
    for form, ci, reg in (("np1", 96, "I"), ("np2", 65, "I"), ("f16s", 128, "Fwx"), ("np3", 96, "I")):
        for act in ("gelu", "exp"):
            o = "y" if act == "exp" and form in ("np1", "f16s") else "yp"               # exp(v) may leave fp16's range: no fp16 planes of it
            out.append(_with_act(Case(form, tag="act", n=2, t=70, ci=ci, co=137, regime=reg, out=o), act))
        out.append(_with_act(Case(form, tag="act", n=2, t=70, ci=ci, co=137, regime=reg, out="yp", ep=EP, alias=form != "np1"), "gelu"))
    # exp into an fp16 plane where the bound of v keeps it in range: sum |w| |x| + |b| <= 128 * 5 / 64 + 4 / 64 < ln 65504
    out.append(Case("kb2", tag="act", n=2, t=70, ci=128, co=137, act="exp", xa=1, wa=5, wexp=-6, out="yp"))
    return out


def network_cases():
    """the three uses of the fp16 split form in csrc/networks.hip, and the argmax on three planes"""
    F = lambda **k: Case("f16s", regime="Fwx", **k)
    out = [F(tag="pw1", n=2, t=150, ci=64, co=200, act="gelu", out="p"),                  # GELU, planes only, scaled by pout_scale
           F(tag="pw2", n=2, t=150, ci=160, co=64, ep=("bias", "ch_scale", "residual"), alias=True, out="y"),
           F(tag="pw2", n=3, t=37, ci=97, co=65, ep=("bias", "ch_scale", "residual"), alias=True, out="y"),
           F(tag="classifier", n=1, t=130, ci=128, co=4096, act="argmax", out="a"),
           F(tag="classifier", n=3, t=37, ci=33, co=200, act="argmax", out="a"),
           Case("f16s", tag="narrow", n=1, t=129, ci=2, co=130, act="argmax", out="a", xa=1, wa=1, ep=()),
           Case("np3", tag="classifier", n=1, t=129, ci=96, co=200, act="argmax", out="a", regime="IIw"),
           Case("np3", tag="classifier", n=3, t=37, ci=33, co=321, act="argmax", out="a", regime="IIIw"),
           Case("np3", tag="narrow", n=1, t=130, ci=1, co=130, act="argmax", out="a", xa=1, wa=1, ep=())]
    return out


_FORM5 = ("np1", "kb2", "np2", "f16s", "np3")
_EDGE_CI = {"np1": 65, "kb2": 128, "np2": 33, "f16s": 64, "np3": 65}
_EDGE_REG = {"np1": "I", "kb2": "Hx", "np2": "IIwx", "f16s": "Fwx", "np3": "IIx"}


def edge_cases():
    out = []
    rot = ("y", "yp", "p")
    kinds = ((1, False), (2, False), (2, True), (3, False))

    def auto(planes, f16s, **k):
        form = dispatch(planes, f16s, k["n"], k["t"], k["ci"], k["co"])
        reg = {"np1": ("I", "Hw"), "kb2": ("I", "Hx"), "np2": ("IIwx", "IIw"), "f16s": ("Fwx", "Fx"), "np3": ("IIx", "IIIw")}[form][len(out) % 2]
        return Case(form, regime=reg, out=rot[len(out) % 3], **k)

    for i, co in enumerate(CO_EDGES):                               # the co_pad16 clamp of the W rows, full_rows false, rows past pad32(Co)
        for q in range(2):
            pl, fs = kinds[(i + 2 * q) % 4]
            out.append(auto(pl, fs, tag="co", n=2, t=70, ci=(40, 128)[q], co=co))
    for i, ci in enumerate(CI_EDGES):
        for q in range(2):
            pl, fs = kinds[(i + 1 + 2 * q) % 4]
            out.append(auto(pl, fs, tag="ci", n=1, t=130, ci=ci, co=(40, 137)[q]))
    for i, (n, t) in enumerate(((1, 1), (3, 37), (1, 127), (1, 128), (1, 129), (2, 150))):     # a tile across batch items; T > 128, 3 column tiles
        for q in range(4):
            pl, fs = kinds[q]
            out.append(auto(pl, fs, tag="cols", n=n, t=t, ci=(104, 40)[(i + q) % 2], co=(65, 137)[(i + q) % 2]))
    for i, ep in enumerate(EP_SUBSETS):                             # every subset of the epilogue, on two forms each
        for q, form in enumerate((_FORM5[i % 5], _FORM5[(i + 2) % 5])):
            o = rot[(i + q) % 3]
            alias = "residual" in ep and o != "p" and (i + q) % 2 == 0
            out.append(Case(form, tag="ep", n=2, t=70, ci=_EDGE_CI[form], co=137, regime=_EDGE_REG[form], ep=ep, alias=alias, out=o))
    return out


def persistent_cases():
    """gemm_planes_lw_kernel: Co about 4096 x 16 - 17 column tiles, 3 / 4 / 5 steps = every residue of the ring position at a seam"""
    L = lambda **k: Case("np3lw", **k)
    return [
        L(tag="seam", n=1, t=2048, ci=96, co=4096, regime="I", out="y"),                                   # 512 tiles, nsteps == NS
        L(tag="seam", n=3, t=700, ci=128, co=4100, regime="IIw", out="yp", ep=EP, alias=True),              # 33 x 17 = 561 tiles (& 7 = 1), Co % 32 = 4, ragged columns, stage_small
        L(tag="seam", n=1, t=2050, ci=160, co=4100, regime="IIIw", out="y"),                                # 5 steps; the third plane across the seams
        L(tag="seam", n=2, t=1025, ci=129, co=4097, regime="IIIx", out="p"),                                # planes only
        L(tag="seam", n=1, t=2049, ci=97, co=4133, regime="I", act="argmax", out="a"),                      # 4 steps
        _with_act(L(tag="seam", n=1, t=2050, ci=96, co=4100, regime="I", out="yp"), "gelu"),
    ]


def all_cases():
    return step_cases() + act_cases() + network_cases() + edge_cases() + persistent_cases()
